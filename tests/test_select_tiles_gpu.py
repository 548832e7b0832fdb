"""The three-kernel selection (count, offsets, compact) of the window scan (aln_scan_*) and of the sequence set (aln_seqset_*) on
inputs whose kept set is known by construction (tests/select_cases.py; tests/test_select_tiles_cpu.py checks the construction against
the oracle): hits on thread and tile edges, empty tiles, more than 256 tiles (the offsets kernel's second trip), capacity cuts inside
and between tiles, failed pairs in far tiles, chunks of several tiles that end off a tile edge, and frequency sums over lists beyond
the frequency kernel's grid cap.  Index lists are compared whole; f is compared bit for bit with the oracle's f of the window's or
pair's content, by table lookup."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from aligner_amd import _ffi, runtime, repeats as R                               # noqa: E402
from aligner_amd.batch import RESULT_DTYPE                                        # noqa: E402
from aligner_amd.enums import DNA, Protein                                        # noqa: E402
from aligner_amd.pwm import PWMAlignment, align_window_offsets                    # noqa: E402
from aligner_amd.seqset import SeqSet                                             # noqa: E402
import repeats_held_backend as H                                                  # noqa: E402
import select_cases as SC                                                         # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARY = ("f", "score", "end_y", "end_x", "start_y", "start_x", "aln_len", "status")
GUARD = 8
PATTERN = 0xA5C3F00D


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------- scan
_scan_oracle = {}


def scan_oracle(orc):
    """Per window content (a run of 0 .. 8 ones): the oracle's f and the frequency matrix of its alignment.  Nine calls, once."""
    if not _scan_oracle:
        m = SC.scan_pwm()
        f, freq = [], []
        for L in range(SC.W + 1):
            r = orc.align_pwm(SC.window_content(L), SC.DEL, SC.EXT, m)
            assert r["status"] == 0
            f.append(r["f"])
            freq.append(PWMAlignment(DNA, r["numbered"], r["qal"], SC.W, r["coords"], r["f"]).get_frequency_matrix())
        _scan_oracle["f"] = np.array(f, dtype=np.float64)
        _scan_oracle["freq"] = np.array(freq)
    return _scan_oracle["f"], _scan_oracle["freq"]


def open_scan(case, reverse):
    """The scan holds the forward strand; a reverse pass sees case.strand when the scan holds its mirror image."""
    return R.ScanBackend().scan(case.strand[::-1].copy() if reverse else case.strand)


def score_pass(sc, case, orc, reverse):
    f = sc.score(SC.scan_pwm(), SC.DEL, SC.EXT, case.first, case.step, case.width, reverse=reverse)
    table, _ = scan_oracle(orc)
    assert len(f) == case.n
    assert np.array_equal(_bits(f), _bits(table[case.runs]))
    return f


def raw_select(sc, case, mean, sd, z_min, cap, reverse=False):
    """aln_scan_select into buffers of the test's own, with GUARD entries behind `cap` preset to a pattern."""
    m = SC.scan_pwm()
    p, keep = runtime.make_params(_ffi.PWM_LOCAL, SC.DEL, SC.EXT, m)
    g = sc._geometry(case.first, case.step, case.width, reverse)
    stride = int(sc.lib.aln_scan_string_stride(sc.h, SC.W, C.byref(g)))
    idx = np.full(cap + GUARD, PATTERN, dtype=np.uint32)
    res = np.full((cap + GUARD) * RESULT_DTYPE.itemsize, 0x5A, dtype=np.uint8)
    tb = np.full(stride * (cap + GUARD), 0x5A, dtype=np.uint8)
    count = C.c_uint64(0)
    sc.generation += 1
    st = sc.lib.aln_scan_select(sc.h, C.byref(p), C.byref(g), float(mean), float(sd), float(z_min), cap, C.byref(count), idx.ctypes.data,
                                res.ctypes.data, tb.ctypes.data)
    count = int(count.value)
    got = min(count, cap)
    assert (idx[got:] == PATTERN).all(), "index words beyond min(count, cap) were written"
    assert (res[got * RESULT_DTYPE.itemsize:] == 0x5A).all() and (tb[got * stride:] == 0x5A).all()
    return st, count, idx[:got].astype(np.int64), res[:got * RESULT_DTYPE.itemsize].view(RESULT_DTYPE), tb, stride


def check_selection(sc, case, f, mean, sd, z_min, want, reverse, held=True):
    """One threshold: the select pass and the held pass both give numpy's list on the pass's own f, which is the predicted one."""
    numpy_idx = SC.numpy_kept(f, mean, sd, z_min)
    assert numpy_idx.tolist() == want.tolist(), (case.name, mean, sd, z_min)
    st, count, idx, res, tb, stride = raw_select(sc, case, mean, sd, z_min, max(len(want), 1) + 3, reverse)
    assert st == _ffi.OK and count == len(want), (case.name, mean, sd, z_min, count, len(want))
    assert np.array_equal(idx, want), (case.name, mean, sd, z_min)
    assert np.array_equal(_bits(res["f"]), _bits(f[want]))
    if held:
        hh = sc.hits(SC.scan_pwm(), SC.DEL, SC.EXT, case.first, case.step, case.width, mean, sd, z_min, reverse=reverse)
        assert len(hh) == len(want) and np.array_equal(hh.idx, want), (case.name, mean, sd, z_min)
        assert np.array_equal(_bits(hh.f), _bits(f[want]))
        return hh
    return None


def check_alignments(case, got, windows):
    """PWMAlignment objects of `windows` against the batch call on the same windows."""
    windows = np.asarray(windows, dtype=np.int64)
    lo = int(windows.min()) * SC.W
    starts, lens = case.starts(windows)
    res, ref = align_window_offsets(case.strand[lo:], starts - np.uint64(lo), lens, SC.DEL, SC.EXT, SC.scan_pwm(), want_traceback=True)
    assert len(got) == len(ref)
    for a, b, k in zip(got, ref, windows):
        assert H.same_alignment(a, b), int(k)
    return res


@pytest.mark.parametrize("reverse", [False, True])
def test_scan_tile_edges_and_thresholds(orc, reverse):
    """(a) 3 tiles and a ragged tail; thresholds that hold exactly, sd = 0, NaN."""
    case, named = SC.case_edges()
    with open_scan(case, reverse) as sc:
        f = score_pass(sc, case, orc, reverse)
        sizes = []
        for (mean, sd, z), min_run in SC.SCAN_THRESHOLDS:
            want = case.kept(min_run) if min_run is not None else np.zeros(0, dtype=np.int64)
            hh = check_selection(sc, case, f, mean, sd, z, want, reverse)
            sizes.append(len(want))
            if min_run == 1:
                assert set(named) <= set(hh.idx.tolist())
                edge = np.flatnonzero(np.isin(hh.idx, named))
                check_alignments(case, hh.alignments(edge), hh.idx[edge])
        assert sizes[0] > sizes[1] > sizes[2] > 0 and sizes[3] == sizes[1] and sizes[4] == sizes[5] == 0


def test_scan_empty_tiles_and_exact_multiple(orc):
    """(b) hits in one tile of four; n an exact multiple of the tile with a hit on the last window."""
    for case in (SC.case_empty_tiles(), SC.case_exact_multiple()):
        with open_scan(case, False) as sc:
            f = score_pass(sc, case, orc, False)
            for (mean, sd, z), min_run in SC.SCAN_THRESHOLDS[:3]:
                want = case.kept(min_run)
                hh = check_selection(sc, case, f, mean, sd, z, want, False)
                if min_run == 1:
                    assert len(hh) == len(case.planted) and hh.idx[-1] == max(case.planted)
                    check_alignments(case, hh.alignments(np.arange(len(hh))), hh.idx)


@pytest.mark.parametrize("reverse", [False, True])
def test_scan_more_than_256_tiles(orc, reverse):
    """(c) 257 tiles and a tail: the offsets kernel's second trip.  The runs of 2 and more: none to a few dozen per tile."""
    case, named = SC.case_many_tiles()
    want = case.kept(2)
    with open_scan(case, reverse) as sc:
        f = score_pass(sc, case, orc, reverse)
        hh = check_selection(sc, case, f, 1.0, 0.5, 2.0, want, reverse)                  # (2 - 1) / 0.5 == 2 exactly
        assert set(named) <= set(hh.idx.tolist())
        far = np.flatnonzero(hh.idx >= SC.TRIP * SC.TILE)
        assert len(far) >= 3 and hh.idx[far[0]] == SC.TRIP * SC.TILE and hh.idx[far[0] - 1] == SC.TRIP * SC.TILE - 1
        near = np.concatenate([[0, far[0] - 1], far])
        res = check_alignments(case, hh.alignments(near), hh.idx[near])
        hs = hh.strings(near)
        for key in SUMMARY:
            assert hs.res[key].tolist() == res[key].tolist(), key


def test_scan_capacity_cuts(orc):
    """(d) the capacity cut between two tiles, one to either side of it, one short of the total, the total."""
    case, named = SC.case_edges()
    want = case.kept(1)
    cuts = SC.capacity_cuts(case)
    assert want[cuts[0] - 1] == SC.TILE - 1 and want[cuts[0]] == SC.TILE
    with open_scan(case, False) as sc:
        f = score_pass(sc, case, orc, False)
        for cap in cuts:
            st, count, idx, res, tb, stride = raw_select(sc, case, 0.0, 1.0, 1.0, cap)
            assert st == (_ffi.ERR_CAPACITY if len(want) > cap else _ffi.OK), cap
            assert count == len(want), cap
            assert np.array_equal(idx, want[:cap]), cap
            starts, lens = case.starts(want[:cap])
            full, _ = align_window_offsets(case.strand, starts, lens, SC.DEL, SC.EXT, SC.scan_pwm(), want_traceback=True, want_alignments=False)
            for key in SUMMARY:
                assert res[key].tolist() == full[key].tolist(), (cap, key)
            assert np.array_equal(_bits(res["f"]), _bits(f[want[:cap]]))


def test_scan_frequencies_beyond_the_grid_cap(orc):
    """(e) more than 16 384 listed hits: more than 16 per workgroup, a short last workgroup, fewer than 1024 workgroups; lists in
    reverse and with repeats."""
    case, named = SC.case_many_tiles()
    want = case.kept(1)
    _, freq = scan_oracle(orc)
    with open_scan(case, False) as sc:
        f = score_pass(sc, case, orc, False)
        hh = check_selection(sc, case, f, 0.0, 1.0, 1.0, want, False)
        n = len(hh)
        assert n > 16384 and n % 16 != 0
        runs = case.runs[hh.idx]
        for name, keep in SC.keep_lists(n).items():
            times = np.bincount(runs[keep], minlength=SC.W + 1).astype(np.float64)
            ref = np.tensordot(times, freq, axes=1)                       # per content: its frequency matrix, times how often it is listed
            got = hh.frequencies(keep)
            assert got.shape == (4, SC.W) and np.array_equal(got, ref), name
        assert hh.frequencies(SC.keep_lists(n)["doubled"]).sum() == (runs.sum() + runs[::3].sum())
        rng = np.random.default_rng(5)
        sample = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, 50)]))
        check_alignments(case, hh.alignments(sample), hh.idx[sample])


# ---------------------------------------------------------------- set
_set_oracle = {}


def set_oracle(orc, blosum62):
    """Per (query content, target content): the oracle's status, f and aligned strings.  25 calls, once."""
    if not _set_oracle:
        codes = [np.asarray(Protein.str_to_vec(s), dtype=np.uint8) for s in SC.CONTENTS]
        n = len(codes)
        f, status, strs = np.zeros((n, n)), np.zeros((n, n), dtype=np.int32), {}
        for a in range(n):
            for b in range(n):
                o = orc.align(orc.CORE_LOCAL, codes[a], codes[b], SC.SET_DEL, SC.SET_EXT, blosum62)
                f[a, b], status[a, b] = o["f"], o["status"]
                strs[(a, b)] = (o["qa"].tobytes(), o["ta"].tobytes(), o["end"])
        _set_oracle.update(f=f, status=status, strs=strs)
    return _set_oracle["f"], _set_oracle["status"], _set_oracle["strs"]


@pytest.fixture(scope="module")
def sset():
    codes = [np.asarray(Protein.str_to_vec(s), dtype=np.uint8) for s in SC.set_strings()]
    with SeqSet(codes) as s:
        yield s


def score_block(sset, orc, blosum62, block):
    """score of a block against the oracle per pair of contents, by table lookup; -> (q, t, f, status) of the pass"""
    q, t, want_f, want_status = SC.block_expect(block)
    of, ostatus, _ = set_oracle(orc, blosum62)
    ids = SC.set_content_ids()
    f, status = sset.score(blosum62, SC.SET_DEL, SC.SET_EXT, SC.to_block(block))
    assert len(f) == len(q) == len(status)
    assert np.array_equal(status, ostatus[ids[q], ids[t]]) and np.array_equal(status, want_status)
    ok = status == SC.OK
    assert np.array_equal(_bits(f[ok]), _bits(of[ids[q], ids[t]][ok])) and np.array_equal(f[ok], want_f[ok])
    return q, t, f, status


def check_hits(sset, orc, blosum62, block, scored, f_min, edges=()):
    """hits(f_min) of a block: the whole list against flatnonzero on the score pass's f and status, strings of the hits next to the
    named pair numbers and of a sample against the oracle"""
    q, t, f, status = scored
    want = SC.expect_hits(f, status, f_min)
    held = sset.hits(blosum62, SC.SET_DEL, SC.SET_EXT, f_min, SC.to_block(block))
    assert len(held) == len(want), (block, f_min, len(held), len(want))
    assert np.array_equal(held.index, want.astype(np.uint64)), (block, f_min)
    assert np.array_equal(_bits(held.f), _bits(f[want]))
    assert np.array_equal(held.q, q[want]) and np.array_equal(held.t, t[want])
    assert (status[want] == SC.OK).all()
    near = []
    for k in edges:                                        # the last hit before pair number k and the first at or after it
        p = int(np.searchsorted(want, k))
        near += [p - 1, p]
    pos = SC.sample_positions(len(held), [p for p in near if 0 <= p < len(held)])
    res, strs = held.strings(pos)
    _, _, ostr = set_oracle(orc, blosum62)
    ids = SC.set_content_ids()
    for j, p in enumerate(pos):
        qa, ta, end = ostr[(ids[held.q[p]], ids[held.t[p]])]
        assert res["status"][j] == SC.OK and res["f"][j] == held.f[p]
        assert (res["end_y"][j], res["end_x"][j]) == end
        assert strs[j][0].tobytes() == qa and strs[j][1].tobytes() == ta, (int(held.q[p]), int(held.t[p]))
    return held


def test_set_full_block_thresholds(sset, orc, blosum62):
    """258 tiles: the marked pairs sit on the tile 0 | 1 and tile 255 | 256 edges and in tile 257; f >= 12 keeps 4 to 240 pairs of
    every tile; the empty sequence's row and column fail in tiles 256 and 257."""
    T = SC.TILE
    scored = score_block(sset, orc, blosum62, ("full",))
    held = check_hits(sset, orc, blosum62, ("full",), scored, SC.F_MARKED, edges=[T, SC.TRIP * T])
    assert len(held) == len(SC.MARKED) ** 2
    assert {T - 1, T, SC.TRIP * T - 1, SC.TRIP * T} <= set(held.index.tolist()) and held.index[-1] // T == SC.TRIP + 1
    held = check_hits(sset, orc, blosum62, ("full",), scored, SC.F_BACKGROUND, edges=[T, 2 * T, SC.TRIP * T, (SC.TRIP + 1) * T])
    assert len(held) > 50000 and (np.bincount((held.index // T).astype(np.int64), minlength=SC.TRIP + 2) > 0).all()


def test_set_everything_kept_but_the_failed_pairs(sset, orc, blosum62):
    """f_min = -inf on the last 8 rows of the grid (2.8 tiles, with the empty sequence's row): every OK pair, no failed one."""
    block = ("rect",) + SC.RECT_TAIL
    scored = score_block(sset, orc, blosum62, block)
    q, t, f, status = scored
    held = check_hits(sset, orc, blosum62, block, scored, float("-inf"), edges=[SC.TILE, 2 * SC.TILE])
    assert len(held) == (status == SC.OK).sum() < len(q)
    assert not (held.q == SC.EMPTY).any() and not (held.t == SC.EMPTY).any()
    assert (np.isin(held.q, SC.MARKED) == np.isin(held.t, SC.MARKED)).all()               # marked x background has no positive cell


def test_set_triangle_and_inner_rectangle(sset, orc, blosum62):
    """The marked-only pass on the upper triangle and on a rectangle whose ranges do not start at 0: pair order of seqset_ref.py."""
    for block, n_hits in ((("upper", 0, SC.S), 21), (("rect",) + SC.RECT_INNER, 16)):
        scored = score_block(sset, orc, blosum62, block)
        held = check_hits(sset, orc, blosum62, block, scored, SC.F_MARKED)
        assert len(held) == n_hits
        assert np.isin(held.q, SC.MARKED).all() and np.isin(held.t, SC.MARKED).all()


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from aligner_amd.enums import Protein
from aligner_amd.matrices import get_blosum62
from aligner_amd.seqset import SeqSet
import select_cases as SC
m = get_blosum62()
with SeqSet([np.asarray(Protein.str_to_vec(s), dtype=np.uint8) for s in SC.set_strings()]) as s:
    print("DIGEST", SC.set_digest(s, m))
    held = s.hits(m, SC.SET_DEL, SC.SET_EXT, SC.F_MARKED, SC.to_block(("full",)))
    print("CHUNKS", (s.stats()["bytes_down"] - 16 * len(held)) // 16)       # a select pass brings back 16 bytes per chunk and per hit
"""


def test_set_chunked_passes_are_byte_identical(sset, blosum62):
    """ALN_CHUNK_CELLS cuts the full block into 5 chunks of about 50 tiles and the triangle into 3, none ending on a tile edge
    (test_select_tiles_cpu.py derives the counts): every chunk after the first selects with k0 != 0 over several tiles.  In a child,
    as in test_seqset_gpu.py; hit lists, summaries and strings hash alike."""
    L = SC.set_lengths()
    q, t, _, _ = SC.block_expect(("full",))
    chunks = SC.chunk_counts(L, q, t, float(SC.chunk_cells()))
    assert len(chunks) >= 3
    env = dict(os.environ, ALN_CHUNK_CELLS=str(SC.chunk_cells()))
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "DIGEST" in out.stdout, out.stdout + out.stderr
    assert int(out.stdout.split("CHUNKS")[1].split()[0]) == len(chunks)
    assert out.stdout.split("DIGEST")[1].split()[0] == SC.set_digest(sset, blosum62)
    held = sset.hits(blosum62, SC.SET_DEL, SC.SET_EXT, SC.F_MARKED, SC.to_block(("full",)))
    assert (sset.stats()["bytes_down"] - 16 * len(held)) // 16 == 1                      # and this process ran one chunk
