"""All-against-all scoring: SeqSet.score and a held hits pass (aln_seqset_*) against align_batch, score only, on the same pairs with
descriptors built on the host.  2 000 random proteins with C5's length distribution (200 .. 2000 residues), BLOSUM62 11 / 2 core
local, all 1 999 000 pairs.  Both paths run in one session, alternating, three runs each; the minimum is the figure and the batch
path's own spread is the noise a difference has to exceed.
usage: python tools/bench_allpairs.py [--n 2000] [--runs 3] [--out profiles/r08_seqset.txt] [--rocprof DIR]
       python tools/bench_allpairs.py --best 10 [--out profiles/r11_best.txt]
--best K: the K best targets per query over the full n x n rectangle instead: SeqSet.best (selection on the device, winners held with
their strings) against SeqSet.score on the same block + numpy.argpartition and a sort per row on the host + align_batch with traceback
on the winners.
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
ap.add_argument("--best", type=int, default=None, metavar="K")
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


def best_case(K):
    """SeqSet.best against score + host selection + align_batch on the winners, alternating; minima."""
    from aligner_amd.seqset import rectangle
    blk = rectangle(0, n, 0, n)
    rect_pairs, rect_cells = n * n, int(lens.sum()) ** 2

    def host_select(f, status):
        g = np.where(status == 0, f, -np.inf).reshape(n, n)
        part = np.argpartition(-g, K - 1, axis=1)[:, :K]
        rows = np.repeat(np.arange(n), K).reshape(n, K)
        order = np.lexsort((part, -g[rows, part]), axis=1)
        return rows[:, 0:1].repeat(K, 1).ravel(), np.take_along_axis(part, order, axis=1).ravel()

    with SeqSet(seqs) as ss:
        say("The %d best targets per query on a resident sequence set: SeqSet.best against SeqSet.score + numpy + align_batch" % K)
        say("%d proteins (C5 lengths, %d residues), the full %d x %d rectangle: %d pairs, %.4g cells; BLOSUM62 11 / 2 core local; %d runs each, alternating"
            % (n, int(lens.sum()), n, n, rect_pairs, rect_cells, a.runs))
        ss.best(S, 11.0, 2.0, K, block=blk)                 # warm: code objects, buffers
        t_best, t_score, t_sel, t_aln, st_best, st_score = [], [], [], [], None, None
        for r in range(a.runs):
            t0 = time.perf_counter(); held = ss.best(S, 11.0, 2.0, K, block=blk); t_best.append(time.perf_counter() - t0)
            if t_best[-1] == min(t_best): st_best = ss.stats()
            t0 = time.perf_counter(); f, status = ss.score(S, 11.0, 2.0, blk); t_score.append(time.perf_counter() - t0)
            if t_score[-1] == min(t_score): st_score = ss.stats()
            t0 = time.perf_counter(); q, t = host_select(f, status); t_sel.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            b = PairBatch(residues, off[q], lens[q].astype(np.uint64), off[t], lens[t].astype(np.uint64))
            won = align_batch(b, _ffi.CORE_LOCAL, 11.0, 2.0, S, want_traceback=True)
            t_aln.append(time.perf_counter() - t0)
        base = [x + y + z for x, y, z in zip(t_score, t_sel, t_aln)]
        # argpartition keeps any of the targets tied at the cut; the check is the rule itself (a full sort per row, outside the timing)
        g = np.where(status == 0, f, -np.inf).reshape(n, n)
        exact = np.sort(np.stack([np.lexsort((np.arange(n), -g[i]))[:K] for i in range(n)]), axis=1)
        same = bool(len(held) == n * K and np.array_equal(held.t.reshape(n, K), exact) and np.array_equal(held.f, g[held.q, held.t]))
        same_f = bool(np.array_equal(np.sort(g[q, t].reshape(n, K), axis=1), np.sort(held.f.reshape(n, K), axis=1))) if len(held) == n * K else False

        def row(name, ts):
            say("%-52s %s  min %.1f  spread %.1f" % (name, " ".join("%.1f" % (1e3 * v) for v in ts), 1e3 * min(ts), 1e3 * (max(ts) - min(ts))))

        say()
        say("wall time per call [ms]")
        row("SeqSet.best (k = %d: %d kept)" % (K, len(held)), t_best)
        row("baseline: score + select + align_batch", base)
        row("  SeqSet.score", t_score)
        row("  numpy.argpartition + sort per row", t_sel)
        row("  align_batch with traceback on the winners", t_aln)
        say()
        say("SeqSet.best:  fill kernels %.1f ms, selection kernels %.2f ms (%.2f %% of the fill), re-fill + walk %.1f ms, %.2f MB up, %.2f MB down"
            % (st_best["fill_ms"], st_best["fetch_kernel_ms"], 100.0 * st_best["fetch_kernel_ms"] / st_best["fill_ms"], st_best["refill_ms"],
               st_best["bytes_up"] / 1e6, st_best["bytes_down"] / 1e6))
        say("SeqSet.score: fill kernels %.1f ms, %.2f MB up, %.2f MB down (12 bytes per pair); the winners' batch: %.2f MB up, %.2f MB down"
            % (st_score["fill_ms"], st_score["bytes_up"] / 1e6, st_score["bytes_down"] / 1e6,
               (32 * len(q) + len(residues)) / 1e6, (48 * len(q) + 2 * int((lens[q] + lens[t] + 2).sum())) / 1e6))
        say("the kept pairs equal the rule applied to the scores (full sort per row): %s; their f equal the host selection's, row by row: %s" % (same, same_f))
        d = min(base) - min(t_best)
        noise = max(max(base) - min(base), max(t_best) - min(t_best))
        say("SeqSet.best against the baseline: %.1f ms %s (the larger spread of the two: %.1f ms)" % (1e3 * abs(d), "less" if d > 0 else "MORE", 1e3 * noise))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if a.best is not None:
    best_case(a.best)
    sys.exit(0)


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
