"""The k best partners per record three ways, on bench_prefilter.py's family workload (2 000 proteins in 200 families of 10, each
family one workloads.random_codes ancestor of a C5 length and nine workloads.mutate copies; BLOSUM62 11 / 2 core local), K = 9,
self pairs skipped, the full square of the set:
  (a) best    SeqSet.best: every pair aligned, selected on the device
  (b) parent  what a caller could do before Candidates.best existed: SeqSet.prefilter + Candidates.score (12 bytes per candidate
              down) + a per-row numpy selection + align_batch on the winners.  Its three library calls are unchanged code
  (c) search  SeqSet.prefilter + Candidates.best: selected on the device, 16 bytes per kept pair down
The prefilter runs as (k, min_shared, min_per_1024) = (3, 0, 256) over the twenty standard residues.  Alternating runs, a process
each (set creation and one warm call of the same kind outside the timing); the runs, median and spread of each, the selection kernels'
own time, bytes up and down, and the recall |hits of (c) & hits of (a)| / |hits of (a)| (reported, never asserted: it belongs to the
thresholds).
usage: python tools/bench_search.py [--families 200] [--runs 3] [--k 9] [--out profiles/r17_search.txt]"""
import argparse, json, os, subprocess, sys, tempfile, time
sys.path.insert(0, ".")
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--families", type=int, default=200)
ap.add_argument("--members", type=int, default=10)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--k", type=int, default=9)
ap.add_argument("--sub-rate", type=float, default=0.15)
ap.add_argument("--indel-rate", type=float, default=0.02)
ap.add_argument("--out", default="profiles/r17_search.txt")
ap.add_argument("--child", default=None, help="(internal) best | parent | search")
ap.add_argument("--work", default=None, help="(internal) the workload and result files' directory")
a = ap.parse_args()
MODES = ["best", "parent", "search"]
NAMES = {"best": "(a) SeqSet.best, every pair", "parent": "(b) prefilter + Candidates.score + numpy selection + align_batch",
         "search": "(c) prefilter + Candidates.best"}
KMER = (3, 0, 256)


def workload():
    from aligner_amd import workloads
    lens = workloads.c5_lengths(a.families)[0]
    seqs = []
    for fam in range(a.families):
        anc = workloads.random_codes(workloads.SEED_C5 + 1000 + fam, int(lens[fam]), 20)
        seqs.append(anc)
        for m in range(1, a.members):
            seqs.append(np.asarray(workloads.mutate(anc, workloads.SEED_C5 + 100000 + fam * 64 + m, 20, a.sub_rate, a.indel_rate), dtype=np.uint8))
    return seqs


def select_rows(index, q, t, f, status, t_count, k):
    """the per-row selection of (b) in numpy: ok pairs off the diagonal, f descending then target ascending, the first k of each row"""
    pos = np.flatnonzero((status == 0) & (f == f) & (q != t))
    row = index[pos] // np.uint64(t_count)
    order = pos[np.lexsort((t[pos], -(f[pos] + 0.0), row))]
    rows = index[order] // np.uint64(t_count)
    start = np.flatnonzero(np.concatenate([[True], rows[1:] != rows[:-1]])) if len(order) else np.zeros(0, dtype=np.int64)
    rank = np.arange(len(order)) - np.repeat(start, np.diff(np.concatenate([start, [len(order)]])))
    return np.sort(order[rank < k])


def child():
    from aligner_amd import _ffi
    from aligner_amd.batch import PairBatch, align_batch
    from aligner_amd.matrices import get_blosum62
    from aligner_amd.seqset import SeqSet, rectangle
    data = np.load(os.path.join(a.work, "workload.npz"))
    seqs = np.split(data["residues"], np.cumsum(data["lens"])[:-1])
    n = len(seqs)
    S = get_blosum62()
    out = {"mode": a.child}
    square = rectangle(0, n, 0, n)
    with SeqSet(seqs) as ss:
        def call():
            t0 = time.perf_counter()
            if a.child == "best":
                held = ss.best(S, 11.0, 2.0, a.k, block=square, skip_self=True)
                out["pass"] = ss.stats()
                index, f = held.index, held.f
            else:
                cand = ss.prefilter(KMER[0], 20, min_shared=KMER[1], min_per_1024=KMER[2], block=square)
                out["share"] = ss.stats()
                out["candidates"] = len(cand)
                if a.child == "search":
                    held = cand.best(S, 11.0, 2.0, a.k, skip_self=True)
                    out["pass"] = ss.stats()
                    index, f = held.index, held.f
                else:
                    cf, cstatus = cand.score(S, 11.0, 2.0)
                    out["pass"] = ss.stats()
                    keep = select_rows(cand.index, cand.q, cand.t, cf, cstatus, n, a.k)
                    res = align_batch(PairBatch.from_pairs((seqs[int(q)], seqs[int(t)]) for q, t in zip(cand.q[keep], cand.t[keep])), _ffi.CORE_LOCAL,
                                      11.0, 2.0, S)
                    index, f = cand.index[keep], np.asarray(res.results["f"], dtype=np.float64)
            out["wall_ms"] = 1e3 * (time.perf_counter() - t0)
            return index, f
        call()                                   # warm: code objects, buffers
        index, f = call()
        out["hits"] = len(index)
        np.savez(os.path.join(a.work, "hits_%s.npz" % a.child), index=index, f=f)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as work:
        seqs = workload()
        lens = np.array([len(s) for s in seqs], dtype=np.int64)
        np.savez(os.path.join(work, "workload.npz"), residues=np.concatenate(seqs), lens=lens)
        n = len(seqs)
        say("the %d best partners per record: SeqSet.best against the prefiltered paths, on a resident sequence set" % a.k)
        say("%d proteins in %d families of %d (ancestor of a C5 length, copies by workloads.mutate: substitutions %.2f, indels %.2f), %d residues"
            % (n, a.families, a.members, a.sub_rate, a.indel_rate, int(lens.sum())))
        say("full square: %d pairs, %.4g cells; BLOSUM62 11 / 2 core local; skip-self; prefilter (k, min_shared, per 1024) = (%d, %d, %d);"
            % (n * n, float(lens.sum()) ** 2, KMER[0], KMER[1], KMER[2]))
        say("%d alternating runs, a process each (warm call outside the timing).  (b)'s three library calls are unchanged code" % a.runs)
        res = {m: [] for m in MODES}
        for r in range(a.runs):
            for m in MODES:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", m, "--work", work, "--k", str(a.k)],
                                     capture_output=True, text=True, timeout=900)
                got = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
                if out.returncode != 0 or not got:
                    say("run %d of %s failed (exit %d): %s" % (r, m, out.returncode, (out.stdout + out.stderr)[-400:]))
                    return 1
                res[m].append(json.loads(got[0][7:]))

        def med(v):
            return float(np.median(v))

        say()
        say("wall time per call [ms]: runs, median, spread (max - min)")
        walls = {}
        for m in MODES:
            w = [x["wall_ms"] for x in res[m]]
            walls[m] = w
            say("%-70s %s  median %.1f  spread %.1f" % (NAMES[m], " ".join("%.1f" % v for v in w), med(w), max(w) - min(w)))
        say()
        for m in MODES:
            x = res[m][-1]
            p = x["pass"]
            extra = "" if m == "best" else "%d candidates of %d pairs (%.3f %%); prefilter %.2f MB down; " % (x["candidates"], n * n, 100.0 * x["candidates"] / (n * n),
                                                                                                         x["share"]["bytes_down"] / 1e6)
            sel = "" if m == "parent" else "selection kernels %.3f ms (median %.3f); " % (p["fetch_kernel_ms"], med([y["pass"]["fetch_kernel_ms"] for y in res[m]]))
            say("%s: %d hits; %sfill kernels %.1f ms; %sthe pass moved %.3f MB up, %.3f MB down"
                % (NAMES[m][:3], x["hits"], extra, p["fill_ms"], sel, p["bytes_up"] / 1e6, p["bytes_down"] / 1e6))
        hits = {m: np.load(os.path.join(work, "hits_%s.npz" % m)) for m in MODES}
        common = np.isin(hits["best"]["index"], hits["search"]["index"])
        say()
        say("recall |(c) & (a)| / |(a)| = %d / %d = %.4f" % (int(common.sum()), len(common), common.sum() / max(len(common), 1)))
        same = np.array_equal(hits["parent"]["index"], hits["search"]["index"]) and np.array_equal(hits["parent"]["f"].view(np.uint64), hits["search"]["f"].view(np.uint64))
        say("(b) and (c) keep the same pairs with the same f bits: %s" % same)
        d = med(walls["parent"]) - med(walls["search"])
        spread = max(walls["parent"]) - min(walls["parent"])
        say("(c) against (b): %.1f ms %s at the median; (b)'s own spread %.1f ms -> %s"
            % (abs(d), "less" if d > 0 else "MORE", spread, "faster beyond the spread" if d > spread else "NOT faster beyond (b)'s spread"))
        say("(c) against (a): %.1f ms against %.1f ms at the median" % (med(walls["search"]), med(walls["best"])))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    if a.child:
        child()
    else:
        sys.exit(main())
