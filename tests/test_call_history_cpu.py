"""The helper of the call-history tests (tests/call_history.py), without a GPU: the schedule covers every ordered pair of
catalogue entries and is the same every time, the catalogue's shapes have the properties that send each entry down its route
(strip counts, the repair condition of the single-pair route, the two-pairs-per-wave condition, the chunk count of the pipelined
entry through aln_plan_chunks), the tag-wrap batches are what the GPU tests take them for, and the comparison rule notices a
difference in every compared field."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import call_history as ch  # noqa: E402
from aligner_amd import _ffi  # noqa: E402

REQUIRED = ["fast_local_long", "fast_local_short", "fast_global", "read_pairs_duo", "claim_runs", "legacy_local_batch", "single_local",
            "single_global", "wg_real", "wg_integer_h_d", "f64_strip_batch", "pwm_fast_windows", "pwm_real_windows", "force_serial",
            "pipelined_four_slots", "shuffle_scores", "scan_hits_held_list"]


def strips(m):
    return (np.asarray(m, dtype=np.int64) + ch.STRIP_ROWS - 1) // ch.STRIP_ROWS


def test_schedule_covers_every_ordered_pair_once():
    for k in (1, 2, 5, 14, 17, 18):
        s = ch.schedule(k)
        assert len(s) == k * k + 1 and s[0] == s[-1]
        assert ch.transitions(s) == {(a, b) for a in range(k) for b in range(k)}
    k = len(ch.catalogue())
    assert 14 <= k <= 18
    s = ch.schedule(k)
    assert len(ch.transitions(s)) == k * k
    # not the catalogue's own order over and over
    assert sum(1 for a, b in zip(s[:-1], s[1:]) if b == (a + 1) % k) == k


def test_schedule_is_deterministic():
    assert ch.schedule(17) == ch.schedule(17)
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import call_history as ch; print(ch.schedule(17))" % (
        os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import subprocess
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == str(ch.schedule(17))


def test_catalogue_is_the_same_every_time():
    a = {e.name: e for e in ch.catalogue()}
    ch._catalogue.clear()
    b = {e.name: e for e in ch.catalogue()}
    assert list(a) == list(b)
    for name in ("fast_local_long", "read_pairs_duo", "f64_strip_batch"):
        assert np.array_equal(a[name].shape["q_len"], b[name].shape["q_len"]) and np.array_equal(a[name].shape["t_len"], b[name].shape["t_len"])


def test_catalogue_shapes_have_the_claimed_properties():
    cat = {e.name: e for e in ch.catalogue()}
    assert list(cat) == REQUIRED
    resident_waves = ch.CUS * 12

    def single_route(n_pairs, N, M):                    # chunk_plan: a large pair, or a sizeable one in a chunk of at most 16
        pc = N.astype(np.int64) * M
        return (N >= 64) & (M >= 128) & ((pc >= 1 << 24) | ((n_pairs <= 16) & (pc >= 1 << 18)))

    for name in ("fast_local_long", "fast_local_short", "fast_global", "read_pairs_duo", "claim_runs", "pipelined_four_slots"):
        s = cat[name].shape
        assert not single_route(len(s["q_len"]), s["q_len"], s["t_len"]).any(), name

    s = cat["fast_local_long"].shape
    assert s["semantics"] == _ffi.CORE_LOCAL and s["dele"] != s["ext"]                 # hazard pairs: three scratch rows
    assert (strips(s["t_len"]) >= 2).all() and len(s["t_len"]) < resident_waves       # multi-strip, passes are shared
    long_max = int(max(s["q_len"].max(), s["t_len"].max()))
    assert 2800 <= long_max <= 3200
    for e in cat.values():                                                             # the longest max_len of the catalogue
        sh = e.shape
        if sh["kind"] == "batch":
            assert max(sh["q_len"].max(), sh["t_len"].max()) <= long_max
        elif sh["kind"] == "pair":
            assert max(sh["N"], sh["M"]) < long_max

    s = cat["fast_local_short"].shape
    assert s["semantics"] == _ffi.CORE_LOCAL and s["dele"] != s["ext"]
    assert 250 <= max(s["q_len"].max(), s["t_len"].max()) <= 300

    s = cat["fast_global"].shape
    assert s["semantics"] == _ffi.CORE_GLOBAL and (strips(s["t_len"]) >= 2).all()

    s = cat["read_pairs_duo"].shape                                                    # aln_fill_duo_kernel's condition
    assert s["semantics"] == _ffi.CORE_GLOBAL and len(s["t_len"]) > resident_waves
    assert s["t_len"].max() <= 256 and s["q_len"].max() <= 1024

    s = cat["claim_runs"].shape
    assert cat["claim_runs"].env == {"ALN_CLAIM": "3"} and len(s["t_len"]) % 3 != 0 and len(s["t_len"]) <= resident_waves
    assert (strips(s["t_len"]) == 1).all() and (s["q_len"].astype(np.int64) * s["t_len"]).max() <= 1 << 18

    assert cat["legacy_local_batch"].shape["semantics"] == _ffi.LEGACY_LOCAL

    s = cat["single_local"].shape                                                      # R = 1 with the localized repair armed
    N, M = np.asarray([s["N"]]), np.asarray([s["M"]])
    assert single_route(1, N, M).all() and s["M"] <= 2560 and "ALN_SINGLE_R" not in cat["single_local"].env
    ns = (s["M"] + 63) // 64
    assert s["semantics"] == _ffi.CORE_LOCAL and s["dele"] != s["ext"] and ns > 8 and s["N"] >= 256 + 64 * 8 + 128

    g = cat["single_global"].shape                                                     # R = 2, another granule stride
    assert single_route(1, np.asarray([g["N"]]), np.asarray([g["M"]])).all() and cat["single_global"].env == {"ALN_SINGLE_R": "2"}
    assert g["semantics"] == _ffi.CORE_GLOBAL and ((g["N"] + 64 + 63) & ~63) != ((s["N"] + 64 + 63) & ~63)

    for name in ("wg_real", "wg_integer_h_d"):                                         # one workgroup per pair (chunk_plan)
        s = cat[name].shape
        assert s["N"] * s["M"] >= 1 << 14 and 16 <= s["N"] <= 8192 and 65 <= s["M"] <= 2048, name

    s = cat["f64_strip_batch"].shape
    assert len(s["t_len"]) == 90 and float(s["dele"]) != int(s["dele"])

    assert ch.planned_chunks(cat["pipelined_four_slots"]) >= 5
    assert "ALN_CHUNK_CELLS" not in os.environ
    for name in ("fast_local_long", "fast_global", "read_pairs_duo", "claim_runs", "f64_strip_batch"):
        assert ch.planned_chunks(cat[name]) == 1, name

    assert cat["shuffle_scores"].shape == dict(kind="shuffle", pairs=3, per_pair=200)
    assert cat["scan_hits_held_list"].shape["length"] == 20000


def test_every_entry_has_an_oracle_answer_within_its_budget(orc):
    import time
    for e in ch.catalogue():
        t0 = time.perf_counter()
        want = e.expected(orc)
        dt = time.perf_counter() - t0
        assert dt < 3.0, (e.name, dt)
        assert any(not k.startswith("_") for k in want), e.name
        assert ch.compare(want, want) is None


def test_tag_wrap_batches():
    a, b, c = ch.wrap_batches()
    for x in (b, c):                                                                   # identical shapes, different residues
        assert np.array_equal(a.q_len, x.q_len) and np.array_equal(a.t_len, x.t_len) and np.array_equal(a.q_off, x.q_off)
        assert not np.array_equal(a.seqs, x.seqs)
    assert not np.array_equal(b.seqs, c.seqs)
    assert (strips(a.t_len) >= 2).all() and ((a.q_len * a.t_len) < (1 << 18)).all() and len(a) <= 16
    assert 1024 % 3 != 0
    pb = ch.pass_batch()
    assert len(pb) >= 22000 and len(pb) / 4 > 4096 * 1.25                              # four fill waves, each beyond the 12-bit count
    assert pb.q_len.min() >= 8 and pb.q_len.max() <= 64 and pb.t_len.min() >= 513 and pb.t_len.max() <= 1100
    assert set(strips(pb.t_len).tolist()) == {2, 3}
    assert 5.0e8 <= pb.cells <= 7.0e8
    ends = np.concatenate([pb.q_off + pb.q_len, pb.t_off + pb.t_len])
    assert int(ends.max()) == len(pb.seqs) and len(np.unique(np.concatenate([pb.q_off, pb.t_off]))) == 2 * len(pb)
    p = _ffi.Params(_ffi.CORE_LOCAL, 0, 11.0, 2.0, None, 24, 24, 24, 3, 98, 0, 0, 0, 0)
    import ctypes as C
    ql, tl = pb.q_len, pb.t_len
    assert _ffi.load().aln_plan_chunks(C.byref(p), ql.ctypes.data, tl.ctypes.data, len(pb), 1, None, None, 0) == 1   # one launch


def test_comparison_rule_sees_every_field():
    want = dict(status=np.zeros(3, np.int32), score=np.arange(3.0), f=np.arange(3.0), end_y=np.arange(3), end_x=np.arange(3),
                start_y=np.arange(3), start_x=np.arange(3), aln_len=np.array([2, 0, 1]), strings=np.arange(6, dtype=np.uint8),
                D=np.zeros((2, 2), np.uint8), H=np.zeros((2, 2)))
    got = {k: v.copy() for k, v in want.items()}
    got["_passes"] = np.array([1, 2, 3])
    assert ch.compare(got, want) is None
    got["_passes"] += 1                                                                # diagnostics: not compared
    assert ch.compare(got, want) is None
    for key in want:
        bad = {k: v.copy() for k, v in got.items()}
        bad[key].flat[-1] += 1
        assert ch.compare(bad, want) is not None and key in ch.compare(bad, want), key
        del bad[key]
        assert ch.compare(bad, want) is not None
    # strings out of the raw buffer, up to aln_len only
    q_len, t_len, aln = np.array([3, 2], np.uint64), np.array([4, 2], np.uint64), np.array([2, 1], np.uint32)
    idx = ch.string_index(q_len, t_len, aln)
    assert idx.tolist() == [0, 1, 9, 10, 18, 24]
    tb = np.arange(40, dtype=np.uint8)
    w2 = dict(aln_len=aln, _idx=idx, strings=tb[idx].copy())
    assert ch.compare(dict(aln_len=aln, _tb=tb), w2) is None
    tb2 = tb.copy(); tb2[2] = 99                                                       # beyond aln_len: not part of the answer
    assert ch.compare(dict(aln_len=aln, _tb=tb2), w2) is None
    tb2[24] = 99
    assert "strings" in ch.compare(dict(aln_len=aln, _tb=tb2), w2)
