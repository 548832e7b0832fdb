"""Held select passes on the GPU (aln_scan_hits / aln_scan_held_*): the hit list, the frequency sums and the strings against
aln_scan_select and the oracle, bit for bit; state errors; the bytes each call moves; the engine on held hits against the engine
on the CPU oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from aligner_amd import _ffi, runtime, repeats as R                               # noqa: E402
from aligner_amd.enums import DNA                                                 # noqa: E402
from aligner_amd.pwm import PWMAlignment                                          # noqa: E402
from repeats_oracle_backend import RecordingBackend                               # noqa: E402
import repeats_held_backend as H                                                  # noqa: E402

pytestmark = pytest.mark.gpu
SUMMARY = ("f", "score", "end_y", "end_x", "start_y", "start_x", "aln_len", "status")
# the widest position-weight matrix the library takes (ALN_MAX_PWM_ENTRIES = 4 x 2000): aln_scan_freq_kernel's counters are 16 bytes
# per column in LDS, 32 000 bytes here, so the kernel has no branch that counts outside LDS and there is no threshold to cross
MAX_PWM_COLS = 2000


def _pwms(W, seed=3):
    rng = np.random.default_rng(seed)
    return {"int": rng.integers(-3, 4, size=(4, W)).astype(np.float64),
            "real": rng.normal(0.0, 1.3, size=(4, W))}


@pytest.fixture(scope="module")
def seq():
    return np.random.default_rng(11).integers(0, 4, 5003).astype(np.uint8)


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64).tolist()


def _same_alignments(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert H.same_alignment(a, b)


def _keep_lists(n):
    every = np.arange(n)
    lists = [every, every[:0], every[::3], every[::-1]]
    if n:
        lists.append(np.array([n - 1, 0, n // 2, 0], dtype=np.int64))        # position 0 twice
    return lists


def _host_sum(alns, keep, W):
    out = np.zeros((4, W), dtype=np.float64)
    for k in keep:
        out = out + alns[int(k)].get_frequency_matrix()
    return out


def _check_pass(sc, m, d, e, first, step, width, mu, s, z, reverse, strings=True):
    """One held pass against one select pass with ample capacity: list, frequencies and strings for every keep list."""
    W = m.shape[1]
    idx, alns = sc.select(m, d, e, first, step, width, mu, s, z, reverse=reverse, cap=sc.windows(first, step, width))
    held = sc.hits(m, d, e, first, step, width, mu, s, z, reverse=reverse)
    assert held.idx.tolist() == idx.tolist(), (mu, s, z)
    assert _bits(held.f) == _bits([a.f for a in alns]), (mu, s, z)
    for keep in _keep_lists(len(idx)):
        got = held.frequencies(keep)
        assert got.shape == (4, W) and got.dtype == np.float64
        assert np.array_equal(got, _host_sum(alns, keep, W)), (mu, s, z, len(keep))
        if strings:
            _same_alignments(held.alignments(keep), [alns[int(k)] for k in keep])
    return idx, alns, held


@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("reverse", [False, True])
def test_held_pass_equals_select_pass(seq, kind, reverse):
    W, first, step, width = 30, 0, 10, 70                     # the cases of test_select_pass_equals_numpy_and_window_batch
    m = _pwms(W, 5)[kind]
    with R.ScanBackend().scan(seq) as sc:
        f = sc.score(m, 4.0, 1.0, first, step, width, reverse=reverse)
        mean, sd = float(np.mean(f)), float(np.std(f))
        cases = [(mean, sd, 1.5), (float(np.median(f)), 0.0, 3.0), (float(f.max()) + 1.0, 1.0, 0.0), (mean, sd, -np.inf)]
        counts = []
        for mu, s, z in cases:
            with np.errstate(divide="ignore", invalid="ignore"):
                want_idx = np.flatnonzero((f - mu) / s >= z)
            idx, alns, held = _check_pass(sc, m, 4.0, 1.0, first, step, width, mu, s, z, reverse)
            assert idx.tolist() == want_idx.tolist(), (mu, s, z)
            counts.append(len(idx))
        assert counts[2] == 0 and counts[3] == len(f) and 0 < counts[0] < len(f)
        # the raw summaries, every field, against select's
        mu, s, z = cases[0]
        sidx, res, tb, count, stride, st = sc.select_raw(m, 4.0, 1.0, first, step, width, mu, s, z, reverse=reverse, cap=len(f))
        assert st == _ffi.OK
        held = sc.hits(m, 4.0, 1.0, first, step, width, mu, s, z, reverse=reverse)
        hs = held.strings(np.arange(count))
        for key in SUMMARY:
            assert hs.res[key].tolist() == res[key][:count].tolist(), key
        for h in range(count):
            L, c = int(res["aln_len"][h]), W + int(held.lengths[h]) + 2
            o = h * stride
            assert hs.stride == stride
            assert np.array_equal(hs.tb[o:o + 4 * L], tb[o:o + 4 * L]) and np.array_equal(hs.tb[o + 4 * c:o + 4 * c + L], tb[o + 4 * c:o + 4 * c + L])


@pytest.mark.parametrize("reverse", [False, True])
def test_held_pass_few_windows_real_pwm(reverse):
    # the four-window geometry of test_few_windows_take_the_batch_calls_routes: the fill takes the one-workgroup route
    seq = np.random.default_rng(21).integers(0, 4, 100).astype(np.uint8)
    W, first, step, width = 300, 0, 30, 330
    m = _pwms(W, 9)["real"]
    with R.ScanBackend().scan(seq) as sc:
        f = sc.score(m, 30.0, 7.0, first, step, width, reverse=reverse)
        mean, sd = float(np.mean(f)), float(np.std(f))
        for mu, s, z in [(mean, sd, -np.inf), (mean, sd, 0.0), (float(f.min()), 0.0, 1.0)]:
            with np.errstate(divide="ignore", invalid="ignore"):
                want_idx = np.flatnonzero((f - mu) / s >= z)
            idx, alns, held = _check_pass(sc, m, 30.0, 7.0, first, step, width, mu, s, z, reverse)
            assert idx.tolist() == want_idx.tolist(), (mu, s, z)


@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("reverse", [False, True])
def test_held_frequencies_short_and_truncated_windows_and_oracle(seq, kind, reverse):
    import oracle
    W, first, step, width = 50, 3, 7, 40                      # windows shorter than the PWM; the last ones truncated
    m = _pwms(W)[kind]
    strand = seq[::-1].copy() if reverse else seq
    with R.ScanBackend().scan(seq) as sc:
        f = sc.score(m, 5.0, 2.0, first, step, width, reverse=reverse)
        mean, sd = float(np.mean(f)), float(np.std(f))
        for z in (1.0, -np.inf):
            idx, alns, held = _check_pass(sc, m, 5.0, 2.0, first, step, width, mean, sd, z, reverse)
            assert len(idx) >= 12
            if z == -np.inf:
                assert held.lengths[-1] < width                  # a truncated window is among the hits
            sample = np.unique(np.linspace(0, len(idx) - 1, 16).astype(int))
            assert len(sample) >= 12
            want = np.zeros((4, W))
            for h in sample:
                j = first + int(idx[h]) * step
                r = oracle.align_pwm(strand[j:min(j + width, len(seq))], 5.0, 2.0, m)
                want = want + PWMAlignment(DNA, r["numbered"], r["qal"], W, r["coords"], r["f"]).get_frequency_matrix()
            assert np.array_equal(held.frequencies(sample), want)


def test_held_frequencies_widest_pwm(seq):
    W, first, step, width = MAX_PWM_COLS, 0, 50, 40            # the most LDS counters a launch asks for
    m = _pwms(W, 13)["int"]
    with R.ScanBackend().scan(seq) as sc:
        f = sc.score(m, 5.0, 2.0, first, step, width)
        idx, alns, held = _check_pass(sc, m, 5.0, 2.0, first, step, width, float(np.mean(f)), float(np.std(f)), -np.inf, False)
        assert len(idx) == len(f) and held.frequencies(np.arange(len(idx))).sum() > 0


class _CountingLib:
    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def _raw_hits(sc, m, d, e, first, step, width, mean, sd, z, reverse=False):
    p, keep = runtime.make_params(_ffi.PWM_LOCAL, d, e, m)
    g = sc._geometry(first, step, width, reverse)
    count = C.c_uint64(0)
    st = sc.lib.aln_scan_hits(sc.h, C.byref(p), C.byref(g), float(mean), float(sd), float(z), C.byref(count))
    return st, int(count.value)


def test_more_hits_than_any_default_capacity_in_one_pass():
    seq = np.random.default_rng(31).integers(0, 4, 50000).astype(np.uint8)
    W, first, step, width = 30, 0, 10, 40
    m = _pwms(W, 7)["int"]
    with R.ScanBackend().scan(seq) as sc:
        n = sc.windows(first, step, width)
        assert n == 5000 and n > sc.cap
        f = sc.score(m, 4.0, 1.0, first, step, width)
        sc.lib = _CountingLib(sc.lib)
        st, count = _raw_hits(sc, m, 4.0, 1.0, first, step, width, 0.0, 1.0, -np.inf)
        assert st == _ffi.OK and count == n
        stats = sc.stats()
        assert stats["fill_ms"] > 0 and stats["refill_ms"] > 0 and stats["d2h_bytes"] == 8
        held = sc.hits(m, 4.0, 1.0, first, step, width, 0.0, 1.0, -np.inf)
        assert sc.lib.calls["aln_scan_hits"] == 2 and "aln_scan_select" not in sc.lib.calls     # one call per pass, none repeated
        assert held.idx.tolist() == list(range(n)) and _bits(held.f) == _bits(f)
        every = np.arange(n)
        got = held.frequencies(every)
        sample = every[::97]
        alns = held.alignments(sample)
        assert np.array_equal(held.frequencies(sample), _host_sum(alns, range(len(alns)), W))
        idx, ref = sc.select(m, 4.0, 1.0, first, step, width, 0.0, 1.0, -np.inf, cap=n)
        assert np.array_equal(got, _host_sum(ref, every, W))
        _same_alignments(alns, [ref[int(k)] for k in sample])


def test_held_state_errors_leave_the_scan_usable(seq):
    W, first, step, width = 30, 0, 10, 70
    m = _pwms(W, 5)["int"]
    with R.ScanBackend().scan(seq) as sc:
        lib = sc.lib
        idx, fbuf, out = np.full(4, 77, dtype=np.uint32), np.full(4, 7.5), np.full((4, W), 7.5)
        keep = np.zeros(1, dtype=np.uint32)
        res, tb = np.zeros(1, dtype=R.RESULT_DTYPE), np.full(4096, 9, dtype=np.uint8)

        def all_refused():
            assert lib.aln_scan_held_list(sc.h, 0, 1, idx.ctypes.data, fbuf.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
            assert lib.aln_scan_held_frequencies(sc.h, keep.ctypes.data, 1, out.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
            assert lib.aln_scan_held_strings(sc.h, keep.ctypes.data, 1, res.ctypes.data, tb.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
            assert idx.tolist() == [77] * 4 and (fbuf == 7.5).all() and (out == 7.5).all() and (tb == 9).all()     # nothing written

        all_refused()                                             # no held state yet
        f = sc.score(m, 4.0, 1.0, first, step, width)
        mean, sd = float(np.mean(f)), float(np.std(f))
        held = sc.hits(m, 4.0, 1.0, first, step, width, mean, sd, 1.5)
        n = len(held)
        assert n > 3
        # positions and ranges beyond the held hits; null pointers with a non-zero length
        bad = np.array([0, n], dtype=np.uint32)
        assert lib.aln_scan_held_frequencies(sc.h, bad.ctypes.data, 2, out.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
        assert lib.aln_scan_held_strings(sc.h, bad.ctypes.data, 2, res.ctypes.data, tb.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
        assert lib.aln_scan_held_list(sc.h, n - 1, 2, idx.ctypes.data, fbuf.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
        assert lib.aln_scan_held_list(sc.h, n + 1, 0, idx.ctypes.data, fbuf.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
        assert lib.aln_scan_held_list(sc.h, 0, 1, None, fbuf.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
        assert lib.aln_scan_held_frequencies(sc.h, None, 1, out.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
        assert lib.aln_scan_held_frequencies(sc.h, keep.ctypes.data, 1, None) == _ffi.ERR_INVALID_ARGUMENT
        assert lib.aln_scan_held_strings(sc.h, keep.ctypes.data, 1, None, tb.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
        assert idx.tolist() == [77] * 4 and (fbuf == 7.5).all() and (out == 7.5).all() and (tb == 9).all()
        with pytest.raises(IndexError):
            held.frequencies([n])
        assert lib.aln_scan_held_list(sc.h, n, 0, None, None) == _ffi.OK          # an empty range at the end is a range
        want = held.frequencies(np.arange(n))                     # the held state survived the refused calls
        sc.score(m, 4.0, 1.0, first, step, width)                 # a score pass replaces it
        all_refused()
        with pytest.raises(RuntimeError):
            held.frequencies(np.arange(n))
        held = sc.hits(m, 4.0, 1.0, first, step, width, mean, sd, 1.5)
        sc.select(m, 4.0, 1.0, first, step, width, mean, sd, 1.5)                 # and so does a select pass
        all_refused()
        held = sc.hits(m, 4.0, 1.0, first, step, width, mean, sd, 1.5)            # the scan is as usable as before
        assert np.array_equal(held.frequencies(np.arange(n)), want)
    assert not hasattr(R.ScanBackend(held=False).scan(seq), "hits")


def test_bytes_moved_by_the_held_calls(seq):
    W, first, step, width = 30, 0, 10, 70
    m = _pwms(W, 5)["real"]
    with R.ScanBackend().scan(seq) as sc:
        f = sc.score(m, 4.0, 1.0, first, step, width)
        mean, sd = float(np.mean(f)), float(np.std(f))
        st, count = _raw_hits(sc, m, 4.0, 1.0, first, step, width, mean, sd, 1.0)
        assert st == _ffi.OK and count > 6
        s = sc.stats()
        assert (s["h2d_bytes"], s["d2h_bytes"]) == (4 * W * 8, 8) and s["fill_ms"] > 0 and s["select_ms"] > 0 and s["refill_ms"] > 0
        g = sc._geometry(first, step, width, False)
        stride = int(sc.lib.aln_scan_string_stride(sc.h, W, C.byref(g)))
        n = count - 2
        idx, fh = np.zeros(n, dtype=np.uint32), np.zeros(n)
        assert sc.lib.aln_scan_held_list(sc.h, 1, n, idx.ctypes.data, fh.ctypes.data) == _ffi.OK
        s = sc.stats()
        assert (s["h2d_bytes"], s["d2h_bytes"]) == (0, 12 * n)
        keep = np.arange(0, count, 2, dtype=np.uint32)
        out = np.zeros((4, W))
        assert sc.lib.aln_scan_held_frequencies(sc.h, keep.ctypes.data, len(keep), out.ctypes.data) == _ffi.OK
        s = sc.stats()
        assert (s["h2d_bytes"], s["d2h_bytes"]) == (4 * len(keep), 32 * W)
        res, tb = np.zeros(len(keep), dtype=R.RESULT_DTYPE), np.zeros(stride * len(keep), dtype=np.uint8)
        assert sc.lib.aln_scan_held_strings(sc.h, keep.ctypes.data, len(keep), res.ctypes.data, tb.ctypes.data) == _ffi.OK
        s = sc.stats()
        assert (s["h2d_bytes"], s["d2h_bytes"]) == (4 * len(keep), len(keep) * (48 + stride))
        assert sc.lib.aln_scan_held_frequencies(sc.h, None, 0, out.ctypes.data) == _ffi.OK and not out.any()
        s = sc.stats()
        assert (s["h2d_bytes"], s["d2h_bytes"]) == (0, 32 * W)


@pytest.mark.parametrize("case", range(3))
def test_engine_on_held_gpu_scan_equals_oracle_engine(case):
    name, raw, opts, seed = H.engine_cases()[case]
    gpu, orc = H.RecordingHeldBackend(R.ScanBackend()), RecordingBackend(H.MemoOracleBackend())
    a = H.run_engine(raw, opts, seed, gpu)
    b = H.run_engine(raw, opts, seed, orc)
    H.assert_same_engine(a, b, gpu.log, orc.log)
    fwd, rev, n_direct, n_inverse = H.case_properties(orc.log, b)
    assert n_direct > 0 and any(n_direct < k for k in fwd), (name, fwd, n_direct)             # some cycle where the filter drops hits
    if name != "flipped":
        assert any(k == 0 and fwd[i - 1] > 0 for i, k in enumerate(fwd) if i), (name, fwd)     # an empty cycle after a non-empty one
    else:
        assert rev and rev[0] > 0 and 0 < n_inverse < rev[0], (name, rev, n_inverse)           # a reverse pass with hits
    # strings came off the device for kept hits only
    assert sum(k for what, n, k in gpu.kept if what == "alignments") < sum(fwd + rev)
    # the select path of the same scan gives the same result
    sel = H.run_engine(raw, opts, seed, R.ScanBackend(held=False))
    for key in a:
        assert len(a[key][0]) == len(sel[key][0]) and np.array_equal(a[key][1], sel[key][1])
        for x, y in zip(a[key][0], sel[key][0]):
            assert (x.left_coord, x.right_coord, x.z) == (y.left_coord, y.right_coord, y.z) and H.same_alignment(x.alignment, y.alignment)


def test_cli_output_is_the_same_on_both_paths(tmp_path):
    raw = H.planted_chromosome(3, 6000, 60)
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">one\n" + raw + b"\n")
    outs = []
    for held in (True, False):
        out = tmp_path / ("held.csv" if held else "select.csv")
        argv = ["-i", str(fa), "-o", str(out), "-r", "60", "-q", "10", "--repeats", "3", "--reverse", "--seed", "5"]
        assert R.main(argv, backend=R.ScanBackend(held=held)) == 0
        outs.append((out.read_bytes(), (tmp_path / (out.name + ".matrices.json")).read_bytes()))
    assert outs[0] == outs[1] and outs[0][0].count(b"\n") > 1
