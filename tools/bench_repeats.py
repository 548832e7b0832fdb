"""The repeat search's window scan against the batch call on the same windows (aln_scan_* vs aln_align_batch).

A seeded synthetic 10 Mb chromosome with planted repeats, a real-valued PWM, the default geometry (windows of 330 rows every 30:
333 334 windows x 300 columns).  Prints the scan's score pass (ms, GCUPS), one select pass split into fill / selection / hit
re-fill + walk / download, the bytes each pass moves, one held pass (aln_scan_hits, then the hit list, the overlap filter on
arrays, the kept hits' frequency sum and their strings, each with its bytes), the same windows through
align_window_offsets(want_traceback=False), and the whole engine (3 cycles + reverse) in wall time on the select path and on the
held path.  `python tools/bench_repeats.py [--mb 10] [--reps 5]`."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aligner_amd import _ffi, runtime, repeats as R      # noqa: E402
from aligner_amd.pwm import align_window_offsets         # noqa: E402


def chromosome(n, seed=1):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 4, n).astype(np.uint8)
    motif = rng.integers(0, 4, 330).astype(np.uint8)
    for p in range(1000, n - 400, max(n // 400, 400)):
        m = motif.copy()
        mut = rng.random(330) < 0.1
        m[mut] = rng.integers(0, 4, int(mut.sum()))
        s[p:p + 330] = m
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n = int(a.mb * 1e6)
    seq = chromosome(n)
    rng = np.random.default_rng(2)
    W, width, step, d, e = 300, 330, 30, 30.0, 7.0
    m = R.transform_matrix(rng.integers(-1, 2, size=(4, W)).astype(np.float64), 0.0, d * e, np.full(4, 0.25))
    starts = np.arange(0, n, step, dtype=np.uint64)
    lens = np.minimum(starts + np.uint64(width), np.uint64(n)) - starts
    cells = float(W) * float(lens.sum())
    out = {"windows": int(len(starts)), "cells": cells}
    with R.ScanBackend().scan(seq) as sc:
        sc.score(m, d, e, 0, step, width)                    # warm: plan, buffers
        ts, fill = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            f = sc.score(m, d, e, 0, step, width)
            ts.append((time.perf_counter() - t0) * 1e3)
            fill.append(sc.stats()["fill_ms"])
        st = sc.stats()
        out["score_pass_ms"] = min(ts)
        out["score_pass_gcups"] = cells / (min(ts) * 1e-3) / 1e9
        out["score_fill_kernel_ms"] = min(fill)
        out["score_bytes"] = {"h2d": st["h2d_bytes"], "d2h": st["d2h_bytes"]}
        mean, sd = float(np.mean(f)), float(np.std(f))
        sc.select(m, d, e, 0, step, width, mean, sd, 3.0)
        t0 = time.perf_counter()
        idx, alns = sc.select(m, d, e, 0, step, width, mean, sd, 3.0)
        out["select_pass_ms"] = (time.perf_counter() - t0) * 1e3
        st = sc.stats()
        out["select_hits"] = int(len(idx))
        out["select_split_ms"] = {"fill": st["fill_ms"], "selection": st["select_ms"], "hit_refill_walk": st["refill_ms"],
                                  "download": st["download_ms"]}
        out["select_bytes"] = {"h2d": st["h2d_bytes"], "d2h": st["d2h_bytes"]}
        # one held pass, call by call (the second of two: buffers and plans are warm)
        p, keepalive = runtime.make_params(_ffi.PWM_LOCAL, d, e, m)
        g = sc._geometry(0, step, width, False)
        count = C.c_uint64(0)
        held, calls = {}, {}

        def timed(name, fn):
            t0 = time.perf_counter()
            r = fn()
            st = sc.stats()
            calls[name] = {"ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": st["refill_ms"], "h2d": st["h2d_bytes"], "d2h": st["d2h_bytes"]}
            return r

        for rep in range(2):
            t_all = time.perf_counter()
            st = timed("hits", lambda: sc.lib.aln_scan_hits(sc.h, C.byref(p), C.byref(g), mean, sd, 3.0, C.byref(count)))
            runtime.raise_for_status(st, "aln_scan_hits")
            s0 = sc.stats()
            held["split_ms"] = {"fill": s0["fill_ms"], "selection": s0["select_ms"], "hit_refill_walk": s0["refill_ms"]}
            nh = int(count.value)
            hidx, hf = np.zeros(nh, dtype=np.uint32), np.zeros(nh)
            timed("held_list", lambda: sc.lib.aln_scan_held_list(sc.h, 0, nh, hidx.ctypes.data, hf.ctypes.data))
            t0 = time.perf_counter()
            j = hidx.astype(np.int64) * step
            kept = R.filter_hits(j, np.minimum(j + width, n), (hf - mean) / sd)
            calls["filter_hits"] = {"ms": (time.perf_counter() - t0) * 1e3}
            k32 = np.ascontiguousarray(kept, dtype=np.uint32)
            fm = np.zeros((4, W))
            timed("held_frequencies", lambda: sc.lib.aln_scan_held_frequencies(sc.h, k32.ctypes.data, len(k32), fm.ctypes.data))
            held["pass_ms"] = (time.perf_counter() - t_all) * 1e3          # hits + list + filter + frequencies: what a cycle needs
            stride = int(sc.lib.aln_scan_string_stride(sc.h, W, C.byref(g)))
            res, tb = np.zeros(len(k32), dtype=R.RESULT_DTYPE), np.zeros(stride * len(k32) + 8, dtype=np.uint8)
            timed("held_strings", lambda: sc.lib.aln_scan_held_strings(sc.h, k32.ctypes.data, len(k32), res.ctypes.data, tb.ctypes.data))
        out["held_pass_ms"] = held["pass_ms"]
        out["held_hits"] = nh
        out["held_kept"] = int(len(kept))
        out["held_split_ms"] = held["split_ms"]
        out["held_calls"] = calls
        # the select path's share of the same work on the host: filter_tasks and the frequency sum of the kept tasks
        t0 = time.perf_counter()
        tasks = R.filter_tasks([R.Task(a, int(k) * step, min(int(k) * step + width, n), (a.f - mean) / sd) for k, a in zip(idx, alns)])
        ms = np.zeros((4, W))
        for t in tasks:
            ms = ms + t.alignment.get_frequency_matrix()
        out["select_host_filter_and_sum_ms"] = (time.perf_counter() - t0) * 1e3
        out["held_equals_select"] = bool(hidx.tolist() == idx.tolist() and np.array_equal(fm, ms) and
                                         [t.left_coord for t in tasks] == j[kept].tolist())
    reuse = {}
    align_window_offsets(seq, starts, lens, d, e, m, want_traceback=False, want_alignments=False, reuse=reuse)
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res, _ = align_window_offsets(seq, starts, lens, d, e, m, want_traceback=False, want_alignments=False, reuse=reuse)
        ts.append((time.perf_counter() - t0) * 1e3)
    out["batch_score_ms"] = min(ts)
    out["batch_score_gcups"] = cells / (min(ts) * 1e-3) / 1e9
    out["batch_bytes"] = {"h2d": int(n + 4 * 8 * len(starts)), "d2h": int(48 * len(starts))}
    out["score_pass_equals_batch"] = bool(np.array_equal(f, res["f"]))
    raw = bytes(b"ATCG"[c] for c in seq)
    opts = R.Options(repeats=3, reverse=True)
    t0 = time.perf_counter()
    r = R.perform_calculation_per_sequence(opts, raw, "synthetic", np.random.default_rng(3), R.ScanBackend(held=False))
    out["engine_3_cycles_reverse_s"] = time.perf_counter() - t0
    out["engine_tasks"] = {k: len(v[0]) for k, v in r.items()}
    t0 = time.perf_counter()
    rh = R.perform_calculation_per_sequence(opts, raw, "synthetic", np.random.default_rng(3), R.ScanBackend(held=True))
    out["engine_held_3_cycles_reverse_s"] = time.perf_counter() - t0
    out["engine_held_tasks"] = {k: len(v[0]) for k, v in rh.items()}
    out["engine_held_equals_select"] = bool(list(r) == list(rh) and all(
        np.array_equal(r[k][1], rh[k][1]) and [(t.left_coord, t.right_coord, t.z) for t in r[k][0]] ==
        [(t.left_coord, t.right_coord, t.z) for t in rh[k][0]] for k in r))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
