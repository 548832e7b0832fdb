"""The generic kernels' row-1 advice passes (do_pair and aln_fill_wgpipe_kernel around adopt_advice_checked, aln_kernels.hip;
DESIGN 4.3 / 4.4) against the CPU model in advice_generic_model.py.

Every line of the model's catalogue -- certified on the CPU by test_advice_generic_cpu.py: one to four passes ending
self-consistent or with harmless flips, the strict-order fall-back, second passes forced by a direction alone and by a value,
deciding flips at x = 2, x = N, columns 63 .. 66 and 127 .. 130, M = 1, M = 2, every rows-per-lane count at 64 R - 63, 64 R - 1
and 64 R, two strips, the one-workgroup route at R = 1, 2, 4 with and without a wrapping ring, integer, dyadic, real-valued,
near-tie and PWM scores -- runs on every route that can take it, the route proved from `flags`:

* the generic integer batch kernel (run_strip, flags & 1; force_generic, more than four pairs per call),
* the f64 batch kernel around run_strip (ALN_F64_OLD=1, read at every call) and around the lean f64 strip (force_f64),
* one pair per call: one workgroup per pair (flags & 4) where aln_wg_route_r takes it, the batch kernel's single wave otherwise,
  integer and f64.

Per pair: `passes & 0x7f` and bit 0x80 equal the model's word exactly, under max_passes 0 (= 4), 1, 2, 3, 4; summary and both
strings equal the oracle's (test_gpu_parity._check_batch), and in the one-pair calls every direction as well (check_pair).
The batches of a scheme hold pairs of one to four passes and the fall-back side by side; both f64 builds give identical
records."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import advice_generic_model as gm  # noqa: E402
from test_gpu_parity import _check_batch, check_pair  # noqa: E402
from aligner_amd import _ffi, runtime  # noqa: E402
from aligner_amd.batch import RESULT_DTYPE, PairBatch  # noqa: E402

pytestmark = pytest.mark.gpu

# route: (arguments of aln_params, environment, integer kernel)
BATCH_ROUTES = {
    "int": (dict(force_generic=True), {}, True),
    "f64_old": (dict(force_f64=True), {"ALN_F64_OLD": "1"}, False),
    "f64_lean": (dict(force_f64=True), {}, False),
}
MAX_PASSES = (0, 1, 2, 3, 4)


def groups():
    """The catalogue by (scheme, gaps): one call has one matrix and one pair of penalties."""
    out = {}
    for e in gm.CATALOGUE:
        out.setdefault((e[6], e[7]), []).append(e)
    return out


GROUPS = groups()


def integer_scheme(scheme, gaps):
    return gm.SCHEMES[scheme][2] and all(float(g).is_integer() for g in gaps)


def padded(entries):
    """At least five pairs per call: four or fewer would go to one workgroup each (aln_wg_route_r: "n <= 4")."""
    reps = -(-5 // len(entries))
    return entries * reps


def pwm_batch(windows, de, ex, S, **kw):
    """pwm.align_window_offsets with the arguments of aln_params passed on (force_generic, force_f64, max_passes)."""
    lib = _ffi.load()
    t_len = np.array([len(w) for w in windows], dtype=np.uint64)
    t_off = np.zeros(len(windows), dtype=np.uint64)
    t_off[1:] = np.cumsum(t_len)[:-1]
    seqs = np.ascontiguousarray(np.concatenate(windows), dtype=np.uint8)
    n, W = len(windows), S.shape[1]
    q_off, q_len = np.zeros(n, dtype=np.uint64), np.full(n, W, dtype=np.uint64)
    p, keep = runtime.make_params(_ffi.PWM_LOCAL, de, ex, S, outputs=_ffi.OUT_SCORE | _ffi.OUT_TRACEBACK, **kw)
    res = np.zeros(n, dtype=RESULT_DTYPE)
    tb_sz = ((np.uint64(5) * (t_len + np.uint64(W + 2)) + np.uint64(3)) // np.uint64(4)) * np.uint64(4)
    tb_off = np.zeros(n, dtype=np.uint64)
    tb_off[1:] = np.cumsum(tb_sz)[:-1]
    tb = np.zeros(int(tb_sz.sum()) + 8, dtype=np.uint8)
    st = lib.aln_align_batch(runtime.context(None), C.byref(p), seqs.ctypes.data, q_off.ctypes.data, q_len.ctypes.data,
                             t_off.ctypes.data, t_len.ctypes.data, n, res.ctypes.data, tb.ctypes.data, tb_off.ctypes.data)
    runtime.raise_for_status(st, "aln_align_batch(PWM)")
    return res


def run_group(orc, key, route, max_passes):
    """One batch call of a (scheme, gaps) group on a batch route; returns [(entry, result record)] after the oracle check."""
    scheme, gaps = key
    kw, _, is_int = BATCH_ROUTES[route]
    entries = padded(GROUPS[key])
    S = gm.SCHEMES[scheme][0]()
    pairs = [gm.entry_pair(e) for e in entries]
    if scheme.startswith("pwm"):
        res = pwm_batch([p[1] for p in pairs], gaps[0], gaps[1], S, max_passes=max_passes, **kw)
        for e, p, r in zip(entries, pairs, res):
            ref = orc.align_pwm(p[1], gaps[0], gaps[1], S)
            assert r["status"] == ref["status"] == 0, e[0]
            assert (r["score"], r["f"], r["end_y"], r["end_x"], r["start_y"], r["start_x"], r["aln_len"]) == \
                   (ref["score"], ref["f"]) + ref["end"] + ref["start"] + (len(ref["numbered"]),), (e[0], route)
    else:
        b = PairBatch.from_pairs([(p[0], p[1]) for p in pairs])
        got = _check_batch(orc, b, _ffi.CORE_LOCAL, gaps[0], gaps[1], S, max_passes=max_passes, **kw)
        res = got.results
        assert (res["status"] == 0).all(), key
    # the generic batch kernel: not the fast one (8), not one workgroup per pair (4), not the single-pair route (2)
    assert ((res["flags"] & 0xe) == 0).all() and ((res["flags"] & 1) == (1 if is_int else 0)).all(), (key, route, res["flags"])
    return list(zip(entries, res)), res


def check_words(rows, route, max_passes):
    bad = []
    for e, r in rows:
        want = gm.prediction(e, max_passes)["word"]
        got = int(r["passes"]) & 0xff
        print(e[0], route, "max_passes", max_passes, "gpu", hex(got), "model", hex(want))
        if got != want:
            bad.append((e[0], route, max_passes, hex(got), hex(want)))
    assert not bad, bad


@pytest.mark.parametrize("max_passes", MAX_PASSES)
@pytest.mark.parametrize("route", sorted(BATCH_ROUTES))
def test_batch_routes_make_the_models_passes(orc, monkeypatch, route, max_passes):
    for k, v in BATCH_ROUTES[route][1].items():
        monkeypatch.setenv(k, v)
    if route != "f64_old":
        monkeypatch.delenv("ALN_F64_OLD", raising=False)
    ran = 0
    for key in GROUPS:
        if route == "int" and not integer_scheme(*key):
            continue
        rows, _ = run_group(orc, key, route, max_passes)
        check_words(rows, route, max_passes)
        ran += len(rows)
    assert ran >= (40 if route == "int" else len(gm.CATALOGUE))


def test_both_f64_builds_give_identical_records(orc, monkeypatch):
    """Every group as one call, pairs of different pass counts sharing waves: the lean f64 strip and run_strip's loop agree in
    every field of every record, `passes` included."""
    for key in GROUPS:
        monkeypatch.delenv("ALN_F64_OLD", raising=False)
        _, lean = run_group(orc, key, "f64_lean", 0)
        monkeypatch.setenv("ALN_F64_OLD", "1")
        _, old = run_group(orc, key, "f64_old", 0)
        for f in ("status", "score", "f", "end_y", "end_x", "start_y", "start_x", "aln_len", "passes", "flags"):
            assert (lean[f] == old[f]).all(), (key, f)
    mixed = {int(gm.prediction(e)["word"]) for e in GROUPS[("pm1", (1.5, 0.5))]}
    assert len(mixed) >= 4                                   # one call holds one to four passes and the fall-back


SINGLE = [(e, kind) for e in gm.CATALOGUE for kind in ("int", "f64") if kind == "f64" or integer_scheme(e[6], e[7])]


@pytest.mark.parametrize("entry,kind", SINGLE, ids=["%s-%s" % (e[0], k) for e, k in SINGLE])
def test_one_pair_per_call_one_workgroup_where_the_route_takes_it(orc, monkeypatch, entry, kind):
    monkeypatch.delenv("ALN_F64_OLD", raising=False)
    name, _, _, M, N, _, scheme, gaps = entry[:8]
    q, t, S, de, ex, pwm = gm.entry_pair(entry)
    kw = dict(force_generic=True) if kind == "int" else dict(force_f64=True)
    wg = gm.wg_route(M, N) is not None and not pwm
    for k in MAX_PASSES:
        if pwm:
            ref = orc.align_pwm(t, de, ex, S, want_matrices=True)
            res, numbered, qal, D, _ = runtime.align_pwm(t, de, ex, S, want_directions=True, max_passes=k, **kw)
            assert res.status == ref["status"] == 0
            assert (res.score, res.f, (res.end_y, res.end_x), (res.start_y, res.start_x)) == (ref["score"], ref["f"], ref["end"], ref["start"])
            assert numbered.tolist() == ref["numbered"].tolist() and qal.tolist() == ref["qal"].tolist()
            assert np.array_equal(D, ref["D"]), name
        else:
            res = check_pair(orc, _ffi.CORE_LOCAL, q, t, de, ex, S, directions_only=True, max_passes=k, **kw)
        assert res is not None
        assert (res.flags & 1) == (1 if kind == "int" else 0), (name, res.flags)
        assert (res.flags & 0xe) == (4 if wg else 0), (name, res.flags)          # one workgroup per pair, or the batch kernel's wave
        want = gm.prediction(entry, k)["word"]
        print(name, kind, "wg" if wg else "wave", "max_passes", k, "gpu", hex(res.passes & 0xff), "model", hex(want))
        assert (res.passes & 0xff) == want, (name, kind, k, hex(res.passes), hex(want))
