"""The fast batch fill's cell in two phases (aln_fast.h: every row's diagonal key from the untouched lane state, then the
chain down the rows, each row's carried cell overwritten in place) against the oracle.  The order of the two phases is all
that protects a row's diagonal input from the row above it, and under an exec mask (ramp quads) the new state goes back
into the old registers without a copy, so the cases are about shapes: target rows that put every R = 1 .. 8 into a last
strip, below strip 0 and in it, and query columns from masked-only strips over a single steady quad to the 64-column
refill edges of the feed rings.  All four semantics of the step: core global (a nucleotide scheme), core local (BLOSUM62
11 / 2 with its row-1 hazard machinery, and a del == ext scheme without it), legacy local (the plain C++ branch of the
cell) and PWM scoring (one window batch); plus homolog pairs whose zero cells and advice flips run the penalty select and
the repair path.  Summaries (the fields bench.py's cpu_baseline compares, and f) and both aligned strings up to aln_len."""
import numpy as np
import pytest

from aligner_amd import _ffi, workloads
from aligner_amd.batch import PairBatch, align_batch
from aligner_amd.pwm import align_window_offsets

pytestmark = pytest.mark.gpu
ROWS = (1, 8, 63, 64, 65, 448, 449, 511, 512, 513, 520, 576, 1023, 1025)
COLS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 66, 127, 128, 129, 200)
NUC = np.where(np.eye(4, dtype=bool), 5.0, -4.0)
FIELDS = ("score", "f", "end_y", "end_x", "start_y", "start_x", "aln_len")


def related(rng, n, m, A):
    """A query of n letters and a target of m letters made of runs copied from it, some letters changed, random letters between
    the runs: alignments that cross strips and chunks, zero cells between them."""
    q = rng.integers(0, A, n).astype(np.uint8)
    t = []
    while len(t) < m:
        L = int(rng.integers(4, 90))
        s = int(rng.integers(0, max(1, n - L)))
        run = q[s:s + L].copy()
        mut = rng.random(len(run)) < 0.08
        run[mut] = rng.integers(0, A, int(mut.sum()))
        t.extend(run.tolist())
        t.extend(rng.integers(0, A, int(rng.integers(0, 8))).tolist())
    return q, np.array(t[:m], dtype=np.uint8)


def shapes():
    return [(n, m) for m in ROWS for n in COLS]


def shape_batch(A, seed):
    rng = np.random.default_rng(seed)
    return PairBatch.from_pairs([related(rng, n, m, A) for n, m in shapes()])


def homolog_batch():
    """Targets that are the query with substitutions and indels: long diagonals, many zero cells off them."""
    pairs = []
    for i, (n, m) in enumerate([(600, 600)] * 6 + [(700, 1100)] * 6):
        q = workloads.random_codes(9100 + i, n, 20)
        pairs.append((q, workloads.mutate(q, 9200 + i, 20, 0.10 + 0.03 * (i % 3), 0.04 + 0.02 * (i % 2), out_len=m)))
    return PairBatch.from_pairs(pairs)


def check_batch(orc, b, sem, dele, ext, matrix, labels, fast=True):
    got = align_batch(b, sem, dele, ext, matrix)
    ref, tb, tb_off = orc.align_batch(sem, b.seqs, b.q_off, b.q_len, b.t_off, b.t_len, dele, ext, matrix, n_threads=8)
    assert len(got) == len(labels)
    for i, case in enumerate(labels):
        r, g = ref[i], got.results[i]
        assert g["status"] == r.status == 0, case
        if fast:                                              # the fast batch kernel, not the single-pair route
            assert g["flags"] & _ffi.FLAG_FAST and not g["flags"] & _ffi.FLAG_SINGLE, (case, int(g["flags"]))
        assert tuple(g[k] for k in FIELDS) == tuple(getattr(r, k) for k in FIELDS), case
        qa, ta = got.aligned(i)
        cap = int(b.q_len[i] + b.t_len[i]) + 2
        o = int(tb_off[i])
        assert (qa == tb[o:o + r.aln_len]).all() and (ta == tb[o + cap:o + cap + r.aln_len]).all(), case
    return got


SCHEMES = {
    "core_global_nucleotide": (_ffi.CORE_GLOBAL, 4, 6, 1, "nuc"),
    "core_local_blosum62_11_2": (_ffi.CORE_LOCAL, 20, 11, 2, "blosum62"),
    "core_local_del_eq_ext": (_ffi.CORE_LOCAL, 20, 5, 5, "blosum62"),
    "legacy_local_blosum62": (_ffi.LEGACY_LOCAL, 20, 11, 2, "blosum62"),
}


@pytest.mark.parametrize("name", list(SCHEMES))
def test_every_last_strip_height_and_column_edge(orc, blosum62, name):
    sem, A, dele, ext, mat = SCHEMES[name]
    b = shape_batch(A, 20261018 + A + dele)
    assert len(b) == len(ROWS) * len(COLS)
    check_batch(orc, b, sem, dele, ext, NUC if mat == "nuc" else blosum62, [(name, "N=%d" % n, "M=%d" % m) for n, m in shapes()])


def test_homolog_pairs_run_the_penalty_select_and_the_repair(orc, blosum62):
    b = homolog_batch()
    labels = [("homolog", i, "N=%d" % int(b.q_len[i]), "M=%d" % int(b.t_len[i])) for i in range(len(b))]
    got = check_batch(orc, b, _ffi.CORE_LOCAL, 11, 2, blosum62, labels)
    assert (got.results["aln_len"] > 300).all()                # the homology was found: the alignments run along the diagonal


def test_pwm_window_batch(orc):
    """Windows of every ROWS length out of one sequence against a 4 x 129 integer PWM (two 64-column chunks and one column)."""
    rng = np.random.default_rng(20261019)
    W = 129
    pwm = rng.integers(-6, 9, (4, W)).astype(np.float64)
    seq = rng.integers(0, 4, 4000).astype(np.uint8)
    # plant the PWM's consensus (with a few changes) so that windows hold a real hit
    cons = pwm.argmax(axis=0).astype(np.uint8)
    for at in (100, 1500, 2900):
        seq[at:at + W] = np.where(rng.random(W) < 0.1, rng.integers(0, 4, W), cons)
    lens = np.array(ROWS, dtype=np.uint64)
    starts = np.array([37 * i + (100 if i % 2 else 1400) for i in range(len(ROWS))], dtype=np.uint64)
    res, alns = align_window_offsets(seq, starts, lens, 5.0, 2.0, pwm)
    for i in range(len(ROWS)):
        s, L = int(starts[i]), int(lens[i])
        ref = orc.align_pwm(seq[s:s + L], 5.0, 2.0, pwm)
        g = res[i]
        assert g["status"] == ref["status"] == 0, L
        assert g["flags"] & _ffi.FLAG_FAST and not g["flags"] & _ffi.FLAG_SINGLE, (L, int(g["flags"]))
        assert (g["score"], g["f"]) == (ref["score"], ref["f"]), L
        assert (g["end_y"], g["end_x"]) == ref["end"] and (g["start_y"], g["start_x"]) == ref["start"], L
        assert g["aln_len"] == len(ref["numbered"]) and alns[i].coords == ref["coords"], L
        assert alns[i].numbered.tolist() == ref["numbered"].tolist() and alns[i].query.tolist() == ref["qal"].tolist(), L
