"""What the batch fill hands on besides its cells (aln_fast.h) against the oracle: the bottom row a strip leaves for the strip
below it -- 64 columns at every 64th step and the rest at the end of the strip (flush_below, flush_tail) -- and the two forms of
core-local strip 0, with the advice feed (re-fills, the localized repair) and without it (a pair's first pass; every pass of a
pair without the row-1 hazard).

Every batch runs on ONE workgroup (ALN_FILL_WGS=1: four waves), so each wave fills several pairs one after the other and what a
pair leaves in the rings and registers is what the next one starts from.

* Flush edges: targets of two to four strips -- 513, 520, 576, 1025 and 1537 rows leave 1, 8, 64, 1 and 1 rows to the last strip
  (R = 1 each: the strip that reads the bottom row is as short as it gets); 640, 900, 1024 and 1536 rows leave 128, 388, 512
  and 512 (R = 2, 7, 8, 8) --, queries on every residue of the tail flush around a 64-step boundary -- no 64-step flush at all, one, two, four.  PWM scoring has strips below strip 0 too (a
  window of more than 512 residues) and a batch of its own here.
* Advice forms: the pairs of advice_model.py's catalogue (routes certified on the CPU by test_advice_model_cpu.py), one batch
  per scheme, the route asserted through aln_pair_result.passes as test_row1_repair_gpu.py does: consistent first passes
  (no feed only), repairs at the first and at later checkpoints (no feed, then the feed, on the same wave), full re-fills
  (the feed for a whole strip 0), with N = 1 and N = 2 pairs among them (step 0's del for row 1; lane 0's compare value going
  from 2 to 1), and a del == ext batch (no hazard: no feed throughout)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import advice_model as am  # noqa: E402
from aligner_amd import _ffi  # noqa: E402
from aligner_amd.batch import PairBatch, align_batch  # noqa: E402
from aligner_amd.pwm import align_window_offsets  # noqa: E402

pytestmark = pytest.mark.gpu
ROWS = (513, 520, 576, 640, 900, 1024, 1025, 1536, 1537)
COLS = (1, 2, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 191, 192, 193, 257)
NUC = np.where(np.eye(4, dtype=bool), 5.0, -4.0)
FIELDS = ("score", "f", "end_y", "end_x", "start_y", "start_x", "aln_len")
SCHEMES = {
    "core_local_blosum62_11_2": (_ffi.CORE_LOCAL, 20, 11, 2, "blosum62"),
    "core_local_del_eq_ext": (_ffi.CORE_LOCAL, 20, 5, 5, "blosum62"),
    "core_global_nucleotide": (_ffi.CORE_GLOBAL, 4, 6, 1, "nuc"),
    "legacy_local_blosum62": (_ffi.LEGACY_LOCAL, 20, 11, 2, "blosum62"),
}


def related(rng, n, m, A):
    """As in test_fill_step_order_gpu.py: a target made of runs copied from the query, some letters changed, random letters
    between the runs -- alignments that cross strip boundaries, so the bottom rows carry more than border values."""
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


@pytest.fixture
def one_workgroup(monkeypatch):
    monkeypatch.setenv("ALN_FILL_WGS", "1")
    monkeypatch.setenv("ALN_NO_SINGLE", "1")


def check_batch(orc, b, sem, dele, ext, matrix, labels):
    got = align_batch(b, sem, dele, ext, matrix)
    ref, tb, tb_off = orc.align_batch(sem, b.seqs, b.q_off, b.q_len, b.t_off, b.t_len, dele, ext, matrix, n_threads=8)
    assert len(got) == len(labels)
    for i, case in enumerate(labels):
        r, g = ref[i], got.results[i]
        assert g["status"] == r.status == 0, case
        assert g["flags"] & _ffi.FLAG_FAST and not g["flags"] & _ffi.FLAG_SINGLE, (case, int(g["flags"]))
        assert tuple(g[k] for k in FIELDS) == tuple(getattr(r, k) for k in FIELDS), case
        qa, ta = got.aligned(i)
        cap = int(b.q_len[i] + b.t_len[i]) + 2
        o = int(tb_off[i])
        assert (qa == tb[o:o + r.aln_len]).all() and (ta == tb[o + cap:o + cap + r.aln_len]).all(), case
    return got


@pytest.mark.parametrize("name", list(SCHEMES))
def test_bottom_row_at_every_flush_edge(orc, blosum62, one_workgroup, name):
    sem, A, dele, ext, mat = SCHEMES[name]
    rng = np.random.default_rng(20261019 + A + dele)
    shapes = [(n, m) for m in ROWS for n in COLS]
    b = PairBatch.from_pairs([related(rng, n, m, A) for n, m in shapes])
    check_batch(orc, b, sem, dele, ext, NUC if mat == "nuc" else blosum62, [(name, "N=%d" % n, "M=%d" % m) for n, m in shapes])


def test_pwm_windows_with_strips_below_strip_0(orc, one_workgroup):
    """PWM scoring can have a strip below strip 0 (windows of 513 .. 1537 residues here).  PWM widths on both sides of a 64-step
    boundary."""
    rng = np.random.default_rng(20261020)
    for W in (63, 65, 129):
        pwm = rng.integers(-6, 9, (4, W)).astype(np.float64)
        seq = rng.integers(0, 4, 4000).astype(np.uint8)
        cons = pwm.argmax(axis=0).astype(np.uint8)
        for at in (100, 700, 1500, 2900):
            seq[at:at + W] = np.where(rng.random(W) < 0.1, rng.integers(0, 4, W), cons)
        lens = np.array(ROWS, dtype=np.uint64)
        starts = np.array([37 * i + (40 if i % 2 else 1400) for i in range(len(ROWS))], dtype=np.uint64)
        res, alns = align_window_offsets(seq, starts, lens, 5.0, 2.0, pwm)
        for i in range(len(ROWS)):
            s, L = int(starts[i]), int(lens[i])
            ref = orc.align_pwm(seq[s:s + L], 5.0, 2.0, pwm)
            g = res[i]
            assert g["status"] == ref["status"] == 0, (W, L)
            assert g["flags"] & _ffi.FLAG_FAST and not g["flags"] & _ffi.FLAG_SINGLE, (W, L, int(g["flags"]))
            assert (g["score"], g["f"]) == (ref["score"], ref["f"]), (W, L)
            assert (g["end_y"], g["end_x"]) == ref["end"] and (g["start_y"], g["start_x"]) == ref["start"], (W, L)
            assert g["aln_len"] == len(ref["numbered"]) and alns[i].coords == ref["coords"], (W, L)
            assert alns[i].numbered.tolist() == ref["numbered"].tolist() and alns[i].query.tolist() == ref["qal"].tolist(), (W, L)


def short_pairs(seed):
    """N = 1 and N = 2 against one, two and three strips, four letters; letter 0 (a match of +1 in both four-letter schemes) opens
    the query and sits in rows 1, M / 2 and M of the target, so every pair has a positive cell."""
    pairs = []
    for M in (5, 64, 513, 1100):
        for N in (1, 2):
            q, t = am.random_pair(M, N, seed + 10 * M + N)
            q[0] = 0
            t[[0, M // 2, M - 1]] = 0
            pairs.append((q, t))
    return pairs


INTERLEAVED = ("planted", (2, 1))                           # the scheme whose batch holds every form
GROUPS = {}
for _e in am.CATALOGUE:
    GROUPS.setdefault((_e[4], _e[5]), []).append(_e)
assert INTERLEAVED in GROUPS


@pytest.mark.parametrize("key", sorted(GROUPS), ids=["%s_%d_%d" % (s, g[0], g[1]) for s, g in sorted(GROUPS)])
def test_advice_forms_pair_after_pair_on_one_wave(orc, one_workgroup, key):
    """One batch per scheme of the catalogue: its consistent, repaired and re-filled pairs and N = 1 / N = 2 pairs share four
    waves, so a wave goes from the form without the feed to the form with it and back, pair after pair."""
    scheme, gaps = key
    entries = GROUPS[key]
    S = am.SCHEMES[scheme]()
    extra = short_pairs(77) if S.shape[0] == 4 else []
    b = PairBatch.from_pairs([am.entry_pair(e)[:2] for e in entries] + extra)
    labels = [e[0] for e in entries] + ["short%d" % i for i in range(len(extra))]
    got = check_batch(orc, b, _ffi.CORE_LOCAL, gaps[0], gaps[1], S, labels)
    routes = set()
    for i, e in enumerate(entries):
        d = am.decode_passes(got.results[i]["passes"])
        assert (d["full"], d["repairs"], d["slot"], d["reason"]) == e[6] and not d["fallback"], (e[0], d)
        routes.add("consistent" if e[6] == (1, 0, 0, 0) else "repaired" if d["full"] == 1 else "refilled")
    for i, (q, t) in enumerate(extra):                        # N = 1: no hazard, one pass; N = 2: never the strict-order fallback
        d = am.decode_passes(got.results[len(entries) + i]["passes"])
        assert not d["fallback"] and (len(q) > 1 or (d["full"], d["repairs"]) == (1, 0)), (labels[len(entries) + i], d)
    if key == INTERLEAVED:                                    # the batch that interleaves every form
        assert routes == {"consistent", "repaired", "refilled"}
        slots = {e[6][2] for e in entries}
        assert 1 in slots and max(slots) == 7                 # repairs at the first and at the last checkpoint


def test_no_hazard_batch_never_feeds_advice(orc, one_workgroup):
    """del == ext: no row-1 hazard, one pass per pair, strip 0 without the feed in every pair -- the catalogue's pairs (zero-rich
    bottom rows) and the short ones under equal gap costs."""
    for scheme in ("planted", "pm1"):
        entries = [e for e in am.CATALOGUE if e[4] == scheme]
        pairs = [am.entry_pair(e)[:2] for e in entries] + short_pairs(99)
        b = PairBatch.from_pairs(pairs)
        got = check_batch(orc, b, _ffi.CORE_LOCAL, 2, 2, am.SCHEMES[scheme](), ["%s_%d" % (scheme, i) for i in range(len(pairs))])
        assert all(am.decode_passes(p) == dict(full=1, fallback=False, repairs=0, slot=0, reason=0) for p in got.results["passes"])
