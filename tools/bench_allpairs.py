"""All-against-all scoring: SeqSet.score and a held hits pass (aln_seqset_*) against align_batch, score only, on the same pairs with
descriptors built on the host.  2 000 random proteins with C5's length distribution (200 .. 2000 residues), BLOSUM62 11 / 2 core
local, all 1 999 000 pairs.  Both paths run in one session, alternating, three runs each; the minimum is the figure and the batch
path's own spread is the noise a difference has to exceed.
usage: python tools/bench_allpairs.py [--n 2000] [--runs 3] [--out profiles/r08_seqset.txt] [--rocprof DIR]
--rocprof DIR: afterwards, one `rocprofv3 --kernel-trace --stats` run of its own (one score pass and one hits pass) into DIR."""
import argparse, csv, glob, os, subprocess, sys, time
sys.path.insert(0, ".")
import numpy as np
from aligner_amd import _ffi, workloads
from aligner_amd.batch import PairBatch, align_batch
from aligner_amd.matrices import get_blosum62
from aligner_amd.seqset import SeqSet

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2000)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default="profiles/r08_seqset.txt")
ap.add_argument("--rocprof", default=None)
ap.add_argument("--once", action="store_true", help="one score pass and one hits pass, nothing else (the run under the profiler)")
a = ap.parse_args()

n = a.n
lens = workloads.c5_lengths(n)[0]
off = np.zeros(n, dtype=np.uint64)
off[1:] = np.cumsum(lens)[:-1]
residues = workloads.random_codes(workloads.SEED_C5 + 7, int(lens.sum()), 20)
seqs = [residues[int(o):int(o) + int(l)] for o, l in zip(off, lens)]
S = get_blosum62()
pairs = n * (n - 1) // 2
cells = int((int(lens.sum()) ** 2 - int((lens.astype(np.int64) ** 2).sum())) // 2)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def batch_descriptors():
    q, t = np.triu_indices(n, 1)
    return PairBatch(residues, off[q], lens[q].astype(np.uint64), off[t], lens[t].astype(np.uint64))


with SeqSet(seqs) as ss:
    if a.once:
        f, status = ss.score(S, 11.0, 2.0)
        held = ss.hits(S, 11.0, 2.0, float(np.quantile(f, 0.99)))
        held.strings(np.arange(min(len(held), 1000), dtype=np.uint32))
        sys.exit(0)
    say("All-against-all scoring on a resident sequence set (aln_seqset_*) against aln_align_batch with host-built descriptors")
    say("%d proteins (C5 lengths, %d residues), %d pairs, %.4g cells; BLOSUM62 11 / 2 core local; %d runs each, alternating"
        % (n, int(lens.sum()), pairs, cells, a.runs))
    f, status = ss.score(S, 11.0, 2.0)                      # warm: code objects, buffers
    f_min = float(np.quantile(f, 0.99))
    t_set, t_hits, t_desc, t_batch, st_score, st_hits = [], [], [], [], None, None
    res = None
    for r in range(a.runs):
        t0 = time.perf_counter(); f, status = ss.score(S, 11.0, 2.0); t_set.append(time.perf_counter() - t0)
        if t_set[-1] == min(t_set): st_score = ss.stats()
        t0 = time.perf_counter(); held = ss.hits(S, 11.0, 2.0, f_min); t_hits.append(time.perf_counter() - t0)
        if t_hits[-1] == min(t_hits): st_hits = ss.stats()
        t0 = time.perf_counter(); b = batch_descriptors(); t_desc.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); res = align_batch(b, _ffi.CORE_LOCAL, 11.0, 2.0, S, want_traceback=False, out=res); t_batch.append(time.perf_counter() - t0)
    same = bool((res.results["f"].view(np.uint64) == f.view(np.uint64)).all() and (res.results["status"] == status).all())
    expect = np.nonzero((status == 0) & (f >= f_min))[0]
    same_hits = bool(len(held) == len(expect) and (held.index == expect.astype(np.uint64)).all())

    def row(name, ts):
        say("%-44s %s  min %.1f  spread %.1f" % (name, " ".join("%.1f" % (1e3 * v) for v in ts), 1e3 * min(ts), 1e3 * (max(ts) - min(ts))))

    say()
    say("wall time per call [ms]")
    row("align_batch, score only (descriptors given)", t_batch)
    row("  building its descriptors (numpy)", t_desc)
    row("SeqSet.score", t_set)
    row("SeqSet.hits (f >= %.0f: %d hits, %.2f %%)" % (f_min, len(held), 100.0 * len(held) / pairs), t_hits)
    say()
    say("GCUPS host to host: align_batch %.0f (%.0f with its descriptors), SeqSet.score %.0f, SeqSet.hits %.0f"
        % (cells / min(t_batch) / 1e9, cells / (min(t_batch) + min(t_desc)) / 1e9, cells / min(t_set) / 1e9, cells / min(t_hits) / 1e9))
    say("SeqSet.score: fill kernels %.1f ms (%.0f GCUPS), %.1f MB up, %.1f MB down" % (st_score["fill_ms"], cells / st_score["fill_ms"] / 1e6,
                                                                                     st_score["bytes_up"] / 1e6, st_score["bytes_down"] / 1e6))
    say("SeqSet.hits:  fill kernels %.1f ms, hit re-fill + walk %.1f ms, %.1f MB up, %.1f MB down" % (st_hits["fill_ms"], st_hits["refill_ms"],
                                                                                                    st_hits["bytes_up"] / 1e6, st_hits["bytes_down"] / 1e6))
    say("align_batch:  %.1f MB up (descriptors %.1f + residues), %.1f MB down" % ((32 * pairs + len(residues)) / 1e6, 32 * pairs / 1e6, 48 * pairs / 1e6))
    say("f and status equal the batch's bit for bit: %s; hits equal the filter of the scores: %s" % (same, same_hits))
    d = min(t_batch) - min(t_set)
    noise = max(t_batch) - min(t_batch)
    say("SeqSet.score against align_batch: %.1f ms %s, %.1f x the batch path's spread (%.1f ms)%s"
        % (1e3 * abs(d), "less" if d > 0 else "MORE", abs(d) / noise if noise > 0 else float("inf"), 1e3 * noise,
           "" if d > noise else " -- not faster beyond the noise"))

if a.rocprof:
    os.makedirs(a.rocprof, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "--", sys.executable, os.path.abspath(__file__), "--n", str(n), "--once"]
    try:
        rc = subprocess.call(cmd, stdout=subprocess.DEVNULL, timeout=240)
    except subprocess.TimeoutExpired:
        rc = 124
    say()
    say("rocprofv3 --kernel-trace --stats, a run of its own (one score pass, one hits pass, strings of up to 1000 hits; exit %d):" % rc)
    if rc != 0:
        say("  the profiled run did not end well: no kernel statistics")
    else:
        for path in sorted(glob.glob(os.path.join(a.rocprof, "**", "*kernel_stats.csv"), recursive=True)):
            for rec in csv.DictReader(open(path)):
                say("  %-48s calls %6s  avg %12.1f us  (%s %%)" % (rec.get("Name", "?")[:48], rec.get("Calls", "?"),
                                                                  float(rec.get("AverageNs", 0)) / 1e3, rec.get("Percentage", "?")))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
