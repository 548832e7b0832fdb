"""The window scan (aln_scan_*) and the repeat-search engine on the GPU: scan passes against align_window_offsets and the
oracle, the engine on the scan against the same engine driven by the CPU oracle, and the CLI end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from aligner_amd import _ffi, repeats as R                                        # noqa: E402
from aligner_amd.pwm import align_window_offsets                                  # noqa: E402
from repeats_oracle_backend import OracleBackend, RecordingBackend                 # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARY = ("f", "score", "end_y", "end_x", "start_y", "start_x", "aln_len", "status")


def _pwms(W, seed=3):
    rng = np.random.default_rng(seed)
    return {"int": rng.integers(-3, 4, size=(4, W)).astype(np.float64),
            "real": rng.normal(0.0, 1.3, size=(4, W))}


def _windows(n, first, step, width):
    starts = np.arange(first, n, step, dtype=np.uint64)
    lens = np.minimum(starts + np.uint64(width), np.uint64(n)) - starts
    return starts, lens


@pytest.fixture(scope="module")
def seq():
    return np.random.default_rng(11).integers(0, 4, 5003).astype(np.uint8)


@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("reverse", [False, True])
def test_score_pass_equals_window_batch_and_oracle(seq, kind, reverse):
    import oracle
    W, first, step, width = 50, 3, 7, 40                      # windows shorter than the PWM; len not a multiple of step
    m = _pwms(W)[kind]
    strand = seq[::-1].copy() if reverse else seq
    starts, lens = _windows(len(seq), first, step, width)
    want, _ = align_window_offsets(strand, starts, lens, 5.0, 2.0, m, want_traceback=False)
    with R.ScanBackend().scan(seq) as sc:
        f = sc.score(m, 5.0, 2.0, first, step, width, reverse=reverse)
    assert len(f) == len(starts)
    assert np.array_equal(f.view(np.uint64), want["f"].view(np.uint64))
    for k in np.linspace(0, len(starts) - 1, 12).astype(int):
        s, L = int(starts[k]), int(lens[k])
        assert f[k] == oracle.align_pwm(strand[s:s + L], 5.0, 2.0, m)["f"], k


@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("reverse", [False, True])
def test_select_pass_equals_numpy_and_window_batch(seq, kind, reverse):
    W, first, step, width = 30, 0, 10, 70
    m = _pwms(W, 5)[kind]
    strand = seq[::-1].copy() if reverse else seq
    starts, lens = _windows(len(seq), first, step, width)
    with R.ScanBackend().scan(seq) as sc:
        f = sc.score(m, 4.0, 1.0, first, step, width, reverse=reverse)
        mean, sd = float(np.mean(f)), float(np.std(f))
        cases = [(mean, sd, 1.5), (float(np.median(f)), 0.0, 3.0), (float(f.max()) + 1.0, 1.0, 0.0), (mean, sd, -np.inf)]
        for mu, s, z in cases:
            with np.errstate(divide="ignore", invalid="ignore"):
                want_idx = np.flatnonzero((f - mu) / s >= z)
            idx, alns = sc.select(m, 4.0, 1.0, first, step, width, mu, s, z, reverse=reverse)
            assert idx.tolist() == want_idx.tolist(), (mu, s, z)
            if len(idx) == 0 or len(idx) > 600:
                continue
            res, ref = align_window_offsets(strand, starts[idx], lens[idx], 4.0, 1.0, m, want_traceback=True)
            for h, k in enumerate(idx):
                a, b = alns[h], ref[h]
                assert a.f == float(res["f"][h]) and a.coords == b.coords, k
                assert a.numbered.tolist() == b.numbered.tolist() and a.query.tolist() == b.query.tolist(), k
        # over capacity: the true count comes back with ERR_CAPACITY, the first `cap` indices are the first hits
        want_idx = np.flatnonzero((f - mean) / sd >= 0.5)
        assert len(want_idx) > 3
        idx, res, tb, count, stride, st = sc.select_raw(m, 4.0, 1.0, first, step, width, mean, sd, 0.5, reverse=reverse, cap=3)
        assert st == _ffi.ERR_CAPACITY and count == len(want_idx)
        assert idx[:3].tolist() == want_idx[:3].tolist()
        full, _ = align_window_offsets(strand, starts[want_idx[:3]], lens[want_idx[:3]], 4.0, 1.0, m, want_traceback=True)
        for key in SUMMARY:
            assert res[key][:3].tolist() == full[key].tolist(), key


@pytest.mark.parametrize("reverse", [False, True])
def test_few_windows_take_the_batch_calls_routes(reverse):
    # <= 4 windows with a real-valued PWM: the long windows take the one-workgroup route, the truncated tail the batch kernel
    seq = np.random.default_rng(21).integers(0, 4, 100).astype(np.uint8)
    W, first, step, width = 300, 0, 30, 330
    m = _pwms(W, 9)["real"]
    strand = seq[::-1].copy() if reverse else seq
    starts, lens = _windows(len(seq), first, step, width)
    assert lens.tolist() == [100, 70, 40, 10]
    want, ref = align_window_offsets(strand, starts, lens, 30.0, 7.0, m, want_traceback=True)
    with R.ScanBackend().scan(seq) as sc:
        for _ in range(2):                                  # the second pass runs on the cached plan
            f = sc.score(m, 30.0, 7.0, first, step, width, reverse=reverse)
            assert np.array_equal(f.view(np.uint64), want["f"].view(np.uint64))
        mean, sd = float(np.mean(f)), float(np.std(f))
        for mu, s, z in [(mean, sd, -np.inf), (mean, sd, 0.0), (float(f.min()), 0.0, 1.0)]:
            with np.errstate(divide="ignore", invalid="ignore"):
                want_idx = np.flatnonzero((f - mu) / s >= z)
            idx, alns = sc.select(m, 30.0, 7.0, first, step, width, mu, s, z, reverse=reverse)
            assert idx.tolist() == want_idx.tolist(), (mu, s, z)
            for h, k in enumerate(idx):
                a, b = alns[h], ref[k]
                assert a.f == float(want["f"][k]) and a.coords == b.coords, k
                assert a.numbered.tolist() == b.numbered.tolist() and a.query.tolist() == b.query.tolist(), k


def test_scan_rejects_other_semantics(seq):
    import ctypes as C
    from aligner_amd import runtime
    lib = _ffi.load()
    with R.ScanBackend().scan(seq) as sc:
        p, keep = runtime.make_params(_ffi.CORE_LOCAL, 5.0, 2.0, np.eye(4))
        g = _ffi.ScanGeometry(0, 10, 40, 0, 0)
        f = np.zeros(lib.aln_scan_windows(sc.h, C.byref(g)))
        assert lib.aln_scan_score(sc.h, C.byref(p), C.byref(g), f.ctypes.data) in (_ffi.ERR_UNSUPPORTED, _ffi.ERR_INVALID_ARGUMENT)


def planted_chromosome(seed, n, rl):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 4, n).astype(np.uint8)
    motif = rng.integers(0, 4, rl + 10).astype(np.uint8)
    for p in range(500, n - rl - 200, n // 14):
        m = motif.copy()
        mut = rng.random(len(m)) < 0.1
        m[mut] = rng.integers(0, 4, int(mut.sum()))
        s[p:p + len(m)] = m
    raw = bytearray(b"ATCG"[c] for c in s)
    raw[3000:3040] = b"N" * 40
    raw[8000:8007] = b"N" * 7
    return bytes(raw)


def _same_engine(raw, opts, seed):
    gpu, orc = RecordingBackend(R.ScanBackend()), RecordingBackend(OracleBackend())
    a = R.perform_calculation_per_sequence(opts, raw, "chr", np.random.default_rng(seed), gpu)
    b = R.perform_calculation_per_sequence(opts, raw, "chr", np.random.default_rng(seed), orc)
    assert list(a) == list(b)
    for key in a:
        ta, ma = a[key]
        tb, mb = b[key]
        assert [(t.left_coord, t.right_coord) for t in ta] == [(t.left_coord, t.right_coord) for t in tb], key
        assert [np.float64(t.z).view(np.uint64) for t in ta] == [np.float64(t.z).view(np.uint64) for t in tb], key
        assert np.array_equal(ma, mb), key
    assert len(gpu.log) == len(orc.log)
    for x, y in zip(gpu.log, orc.log):
        assert x[:5] == y[:5] and x[8] == y[8]
        assert (x[5], x[6]) == (y[5], y[6]) or (np.isnan(x[5]) and np.isnan(y[5]))
        assert np.array_equal(x[7], y[7])
    return gpu.log


def test_engine_equals_oracle_engine_small_geometry():
    raw = planted_chromosome(1, 12000, 60)
    log = _same_engine(raw, R.Options(repeat_length=60, query_offset=10, repeats=3, reverse=True), 101)
    hits = [e[8] for e in log if e[0] == "select" and not e[4]]
    assert sum(1 for h in hits if h) >= 2, hits
    assert any(e[4] for e in log), "the reverse pass ran"


def test_engine_equals_oracle_engine_default_geometry():
    raw = planted_chromosome(2, 20000, 300)
    _same_engine(raw, R.Options(repeats=3, reverse=True), 7)


def test_cli_end_to_end(tmp_path):
    raw1, raw2 = planted_chromosome(3, 6000, 60), planted_chromosome(4, 5000, 60)
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">one\n" + raw1[:3000] + b"\n" + raw1[3000:] + b"\n>two\n" + raw2 + b"\n")
    mask = tmp_path / "m.csv"
    mask.write_text("name,z_value,left_coord,right_coord\none,4.5,100,400\n")
    out = tmp_path / "res.csv"
    p = subprocess.run([sys.executable, "-m", "aligner_amd.repeats", "-i", str(fa), "-o", str(out), "--csv", str(mask), "-r", "60",
                        "-q", "10", "--repeats", "2", "--reverse", "--seed", "5"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Output written to:" in p.stdout and str(out) in p.stdout
    lines = out.read_text().splitlines()
    assert lines[0] == "name,z_value,left_coord,right_coord"
    names = [ln.split(",")[0] for ln in lines[1:]]
    order = {"one": 0, "one-reversed": 1, "two": 2, "two-reversed": 3}
    assert names == sorted(names, key=order.__getitem__)
    import json
    mats = json.loads((tmp_path / "res.csv.matrices.json").read_text())
    assert list(mats) == ["one", "one-reversed", "two", "two-reversed"]
    assert mats["one"]["dim"] == [4, 60] and mats["one"]["v"] == 1
