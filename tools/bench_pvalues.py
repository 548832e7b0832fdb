"""calculate_p_value's batch with the copies drawn on the host against the same batch drawn on the device.

1, 16 and 128 seeded pairs of 350 x 350 (BLOSUM62, 11/2, core local), 4 999 copies each.  Prints one JSON line per size:
  host     calculate_p_value per pair (4 999 shuffle_and_randomize_sequence + PairBatch.from_pairs + one batch call + the fit),
           timed over the first --host-pairs pairs
  device   the aln_shuffle_scores call (device_shuffled_scores: trims on the host, shuffle + fill + gather on the device, 8 bytes
           per copy back), median of --reps warm calls, and its GCUPS over the copies' cells
  fit      calculate_distribution_params + get_p_value per pair on the device call's scores, over the first --fit-pairs pairs
           (some random pairs run the reference's Newton loops to MAXITER: seconds each)
The shuffle kernel's own time is in `rocprofv3 --kernel-trace --stats -- python tools/bench_pvalues.py --host-pairs 0 --fit-pairs 0`
(aln_shuffle_kernel).  `python tools/bench_pvalues.py [--sizes 1,16,128] [--reps 5]`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aligner_amd import statistics                     # noqa: E402
from aligner_amd.batch import PairBatch, align_batch   # noqa: E402
from aligner_amd import _ffi                           # noqa: E402
from aligner_amd.matrices import get_blosum62           # noqa: E402


def pairs_of(n, L=350, seed=1):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 20, L).astype(np.uint8), rng.integers(0, 20, L).astype(np.uint8)) for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-pairs", type=int, default=2)
    ap.add_argument("--fit-pairs", type=int, default=4)
    a = ap.parse_args()
    S = get_blosum62()
    for n in [int(x) for x in a.sizes.split(",")]:
        pairs = pairs_of(n)
        b = PairBatch.from_pairs(pairs)
        init = align_batch(b, _ffi.CORE_LOCAL, 11, 2, S, want_traceback=False).results["f"].astype(np.float64)
        out = {"pairs": n, "copies_per_pair": 4999}
        k = min(n, a.host_pairs)
        if k:
            t0 = time.perf_counter()
            for i in range(k):
                statistics.calculate_p_value(pairs[i][0], pairs[i][1], init[i], 11, 2, S, rng=np.random.default_rng(i))
            out["host_ms_per_pair"] = 1e3 * (time.perf_counter() - t0) / k
        statistics.device_shuffled_scores(b, 11, 2, S, seed=1)                  # warm: buffers, code objects
        ts = []
        for r in range(a.reps):
            t0 = time.perf_counter()
            f, lengths, _ = statistics.device_shuffled_scores(b, 11, 2, S, seed=100 + r)
            ts.append(time.perf_counter() - t0)
        ms = 1e3 * float(np.median(ts))
        cells = float((b.q_len.astype(np.float64)[:, None] * lengths.astype(np.float64)).sum())
        out.update(device_call_ms=ms, device_call_min_ms=1e3 * min(ts), device_gcups=cells / (ms * 1e-3) / 1e9, cells=cells)
        k = min(n, a.fit_pairs)
        if k:
            t0 = time.perf_counter()
            for i in range(k):
                sc = np.concatenate([[init[i]], f[i]])
                ln = np.concatenate([[len(pairs[i][1])], lengths[i].astype(np.int64)])
                statistics.calculate_distribution_params(len(pairs[i][0]), ln, sc).get_p_value(len(pairs[i][0]), len(pairs[i][1]), init[i])
            out["fit_ms_per_pair"] = 1e3 * (time.perf_counter() - t0) / k
            out["device_ms_per_p_value"] = ms / n + out["fit_ms_per_pair"]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
