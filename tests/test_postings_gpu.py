"""What the word join and the seed join share (aln_postings.h, the join skeleton of aln_host.hip) at its edges, both routes over one
tiny set: five records of lengths 0, 3, 40, 0 and 40 at k = 4, so that empty records tie on an offset, one record is shorter than k
and a run of rows has nothing to expand.  An upper block over all five and a rectangle whose first query row is an empty record; one
chunk, and the smallest cap that still admits the fullest row.  Lists exact against wordjoin_ref.py and seedjoin_ref.py, the bytes of
aln_seqset_stats against the formulas that close the two joins in aln_host.hip."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import seedjoin_ref as S                                                        # noqa: E402
import wordjoin_ref as W                                                        # noqa: E402
from aligner_amd.seqset import SeqSet, rectangle, upper                         # noqa: E402

pytestmark = pytest.mark.gpu
K = 4


def records(a):
    rng = np.random.default_rng(40 + a)
    full = rng.integers(0, a, 40).astype(np.uint8)
    twin = full.copy()
    twin[[7, 19, 33]] = (twin[[7, 19, 33]] + 1) % a                              # three substitutions: most words stay shared
    empty = np.zeros(0, dtype=np.uint8)
    return [empty, full[:3].copy(), full, empty.copy(), twin]


def blk_tuple(b):
    return (int(b.q_first), int(b.q_count), int(b.t_first), int(b.t_count), int(b.upper))


@pytest.mark.parametrize("a", [4, 20])
@pytest.mark.parametrize("route", ["word", "seed"])
def test_both_routes_over_the_shared_edges(route, a):
    seqs = records(a)
    assert [len(s) for s in seqs] == [0, 3, 40, 0, 40]
    seen_chunks = set()
    with SeqSet(seqs) as ss:
        if route == "word":
            ss.word_index(K, a)
        else:
            assert ss.seed_index(K, a) == sum(len(ps) for s in seqs for ps in S.positions(s, K, a).values())
        for blk in (upper(0, 5), rectangle(0, 5, 0, 5)):
            bt = blk_tuple(blk)
            rows = W.row_occurrences(seqs, K, a, bt) if route == "word" else S.seed_join(seqs, K, a, band=3, block=bt)[2]
            assert max(rows) > 0 and rows[0] == rows[1] == rows[3] == 0             # the empty and the short record expand nothing
            for cap in (0, max(rows)):
                if route == "word":
                    cand = ss.word_join(K, a, min_shared=1, min_per_1024=0, block=blk, chunk_occurrences=cap)
                    want = W.word_join(seqs, K, a, 1, 0, bt)
                    cut = W.cut(rows, cap if cap else W.CHUNK_OCCURRENCES)
                    chunks = sum(1 for f, n in cut if sum(rows[f:f + n]))
                    got = (cand.index.tolist(), cand.q.tolist(), cand.t.tolist(), cand.shared.tolist())
                    down = 8 * len(rows) + 12 * chunks + 12 * len(cand)
                else:
                    cand = ss.seed_join(K, a, min_seeds=1, band=3, block=blk, chunk_seeds=cap)
                    want, summary, _ = S.seed_join(seqs, K, a, min_seeds=1, band=3, block=bt, chunk_seeds=cap)
                    chunks = summary["chunks"]
                    assert cand.summary == summary
                    got = (cand.index.tolist(), cand.q.tolist(), cand.t.tolist(), cand.shared.tolist(), cand.diag.tolist())
                    down = 8 * len(rows) + 4 + 16 * chunks + 16 * len(cand)
                assert got == tuple(list(x) for x in want), (bt, cap)
                assert len(cand) >= 1
                assert ss.stats()["bytes_down"] == down, (bt, cap)
                seen_chunks.add(chunks)
    assert seen_chunks == {1, 2}                                                    # the rectangle at the small cap: empty row 3 between its chunks
