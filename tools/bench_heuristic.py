"""The heuristic loop for many pairs at once: heuristic.align_many (one resident pair set, per-pair matrices) with each transform
(numpy and native on the host, resident on the device), split into fill, transform kernel, transfers and host transform; a loop of single HeuristicAligner calls on a sample of the same pairs; and one
aln_pairset_run against aln_align_batch (f64 kernels forced) on the same pairs with one shared matrix.
usage: python tools/bench_heuristic.py [n=2000] [sample=200]"""
import sys, time
sys.path.insert(0, ".")
import numpy as np
from aligner_amd import _ffi, heuristic
from aligner_amd.batch import PairBatch, align_batch
from aligner_amd.enums import Protein
from aligner_amd.matrices import get_blosum62
from aligner_amd.pairset import PairSet
from aligner_amd.simple import Heuristics

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
sample = int(sys.argv[2]) if len(sys.argv) > 2 else 200
rng = np.random.default_rng(2025)
pairs, hs = [], []
for k in range(n):
    nq, nt = int(rng.integers(200, 2001)), int(rng.integers(200, 2001))
    q, t = rng.integers(0, 20, nq).astype(np.uint8), rng.integers(0, 20, nt).astype(np.uint8)
    L = int(rng.integers(100, min(nq, nt)))
    a, b = int(rng.integers(0, nq - L + 1)), int(rng.integers(0, nt - L + 1))
    piece = q[a:a + L].copy()
    mut = rng.random(L) < rng.uniform(0.1, 0.5)
    piece[mut] = rng.integers(0, 20, int(mut.sum()))
    t[b:b + L] = piece
    pairs.append((q, t))
    hs.append(Heuristics(float(rng.choice([-0.2, -0.5, -1.0])), 576.0, np.bincount(t, minlength=24).astype(np.float64) / nt))
S = get_blosum62()
cells = sum(len(q) * len(t) for q, t in pairs)
print("%d pairs, %.3g cells per iteration" % (n, cells))

acc = {}


class Timed(PairSet):
    def _t(self, name, fn, *a, **kw):
        t0 = time.perf_counter(); r = fn(*a, **kw); dt = time.perf_counter() - t0
        st = self.stats()
        acc[name] = acc.get(name, 0.0) + dt
        run = name in ("run", "run_stored")
        acc["kernels"] = acc.get("kernels", 0.0) + ((st["fill_ms"] + st["traceback_ms"] if run else 0.0) + st["fetch_kernel_ms"]) * 1e-3
        if name == "reestimate":
            acc["transform_kernel"] = acc.get("transform_kernel", 0.0) + st["fetch_kernel_ms"] * 1e-3
        acc["bytes"] = acc.get("bytes", 0) + st["bytes_up"] + st["bytes_down"]
        acc["up"] = acc.get("up", 0) + st["bytes_up"]
        acc["down"] = acc.get("down", 0) + st["bytes_down"]
        if run:
            acc["run"] = acc.get("run", 0.0) + (dt if name != "run" else 0.0)
            acc["runs"] = acc.get("runs", 0) + 1
            acc["pair_runs"] = acc.get("pair_runs", 0) + len(a[5] if name == "run" else a[4])
        return r

    def run(self, *a, **kw): return self._t("run", PairSet.run, self, *a, **kw)
    def frequencies(self, *a): return self._t("frequencies", PairSet.frequencies, self, *a)
    def strings(self, *a): return self._t("strings", PairSet.strings, self, *a)
    def set_heuristics(self, *a): return self._t("set_heuristics", PairSet.set_heuristics, self, *a)
    def reestimate(self, *a, **kw): return self._t("reestimate", PairSet.reestimate, self, *a, **kw)
    def run_stored(self, *a, **kw): return self._t("run_stored", PairSet.run_stored, self, *a, **kw)
    def matrices(self, *a): return self._t("matrices", PairSet.matrices, self, *a)


inner = heuristic._transform_batch
def timed_transform(*a):
    t0 = time.perf_counter(); r = inner(*a); acc["transform"] = acc.get("transform", 0.0) + time.perf_counter() - t0
    return r
heuristic._transform_batch = timed_transform

results = {}
for how in ("numpy", "native", "resident"):
    for rep in range(2):                      # the second run is reported (buffers and code objects warm)
        acc.clear()
        t0 = time.perf_counter()
        results[how] = heuristic.align_many(pairs, 11.0, 2.0, S, hs, Protein, transform=how, backend=Timed)
        wall = time.perf_counter() - t0
    calls = sum(acc.get(k, 0) for k in ("run", "frequencies", "strings", "set_heuristics", "reestimate", "matrices"))
    host = acc.get("transform", 0.0)
    print("align_many %-8s: %8.1f ms wall = %7.1f kernels (of them %6.2f transform kernel) + %7.1f transfers and call overhead + %7.1f host "
          "transform + %7.1f driver; %d runs, %d pair-runs, %.1f ms per run, %.1f MB moved, per pair-run %.0f bytes up, %.0f down"
          % (how, wall * 1e3, acc["kernels"] * 1e3, acc.get("transform_kernel", 0.0) * 1e3, (calls - acc["kernels"]) * 1e3, host * 1e3,
             (wall - calls - host) * 1e3, acc["runs"], acc["pair_runs"], wall * 1e3 / acc["runs"], acc["bytes"] / 1e6,
             acc["up"] / acc["pair_runs"], acc["down"] / acc["pair_runs"]))
same = all(a.alignment.f == b.alignment.f and a.matrix.tobytes() == b.matrix.tobytes() and a.matrix.tobytes() == c.matrix.tobytes()
           and a.alignment.query.tobytes() == c.alignment.query.tobytes()
           for a, b, c in zip(results["numpy"], results["native"], results["resident"]))
print("numpy, native and resident transforms give the same results: %s" % same)

idx = rng.choice(n, min(sample, n), replace=False)
t0 = time.perf_counter()
single = [heuristic.HeuristicAligner.from_seqs(pairs[i][0], pairs[i][1], Protein).perform_alignment(11.0, 2.0, S, hs[i]) for i in idx]
dt = time.perf_counter() - t0
ok = all(single[k].alignment.f == results["numpy"][i].alignment.f for k, i in enumerate(idx))
print("single HeuristicAligner calls, %d of the pairs: %.1f ms = %.3f ms per pair (equal f: %s)" % (len(idx), dt * 1e3, dt * 1e3 / len(idx), ok))

# one run under one shared real-valued matrix: the pair set against the batch call
M = S * 0.37 + 0.013
b = PairBatch.from_pairs(pairs)
r = None
best_b = 1e9
for i in range(4):
    t0 = time.perf_counter(); r = align_batch(b, _ffi.CORE_LOCAL, 11.3, 2.1, M, want_traceback=True, out=r, force_f64=True); best_b = min(best_b, time.perf_counter() - t0)
mats = np.array([M] * n)
act = np.arange(n, dtype=np.uint32)
with PairSet(b) as ps:
    best_p, kern = 1e9, 0
    for i in range(4):
        t0 = time.perf_counter(); res = ps.run(_ffi.CORE_LOCAL, 11.3, 2.1, mats, act); dt = time.perf_counter() - t0
        if dt < best_p: best_p, kern = dt, ps.stats()["fill_ms"] + ps.stats()["traceback_ms"]
print("one shared matrix: aln_align_batch (f64) %.1f ms = %.0f GCUPS host to host; aln_pairset_run %.1f ms = %.0f GCUPS (kernels %.1f ms = %.0f GCUPS), "
      "summaries equal: %s" % (best_b * 1e3, cells / best_b / 1e9, best_p * 1e3, cells / best_p / 1e9, kern, cells / kern / 1e6,
                               res.tobytes() == r.results.tobytes()))
