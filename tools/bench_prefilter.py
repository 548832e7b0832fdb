"""The k-mer prefilter against the unfiltered held pass: SeqSet.hits(f_min) on the upper block against SeqSet.prefilter +
Candidates.hits(f_min), on 2 000 proteins in 200 families of 10 -- each family one workloads.random_codes ancestor of a C5 length
(200 .. 2000 residues) and nine workloads.mutate copies of it (substitution rate 0.15, indel rate 0.02).  BLOSUM62 11 / 2 core local.
The prefilter runs as (k, min_shared, min_per_1024) = (3, 0, 256) and (4, 8, 128) over the twenty standard residues.  Three alternating
runs, a process each (set creation and one warm call of the same kind outside the timing); median and spread of each, the index and
sharing kernels' own time, the candidate count, the recall |candidate hits| / |full hits| (reported, never asserted: it belongs to the
thresholds), bytes moved.
f_min: unless given, halfway between the highest f of a pair from two families and the lowest f of a pair within one, found by a
probe pass of SeqSet.score in a process of its own before the timed runs.
usage: python tools/bench_prefilter.py [--families 200] [--runs 3] [--f-min F] [--out profiles/r16_prefilter.txt]"""
import argparse, json, os, subprocess, sys, tempfile, time
sys.path.insert(0, ".")
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--families", type=int, default=200)
ap.add_argument("--members", type=int, default=10)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--f-min", type=float, default=None, help="default: halfway between the best pair of two families and the worst pair within one (a probe pass of SeqSet.score finds them)")
ap.add_argument("--sub-rate", type=float, default=0.15)
ap.add_argument("--indel-rate", type=float, default=0.02)
ap.add_argument("--out", default="profiles/r16_prefilter.txt")
ap.add_argument("--child", default=None, help="(internal) full | k,min_shared,min_per_1024")
ap.add_argument("--work", default=None, help="(internal) the workload and result files' directory")
a = ap.parse_args()
MODES = ["full", "3,0,256", "4,8,128"]


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


def child():
    from aligner_amd.matrices import get_blosum62
    from aligner_amd.seqset import SeqSet
    data = np.load(os.path.join(a.work, "workload.npz"))
    seqs = np.split(data["residues"], np.cumsum(data["lens"])[:-1])
    S = get_blosum62()
    out = {"mode": a.child}
    with SeqSet(seqs) as ss:
        if a.child == "probe":
            f, status = ss.score(S, 11.0, 2.0)
            q, t = np.triu_indices(len(seqs), 1)
            same = (q // a.members) == (t // a.members)
            print("RESULT " + json.dumps({"within_min": float(f[same].min()), "within_median": float(np.median(f[same])), "across_max": float(f[~same].max()),
                                          "across_median": float(np.median(f[~same])), "failed": int((status != 0).sum())}), flush=True)
            return

        def call():
            if a.child == "full":
                t0 = time.perf_counter()
                held = ss.hits(S, 11.0, 2.0, a.f_min)
                out["wall_ms"] = 1e3 * (time.perf_counter() - t0)
                out["pass"] = ss.stats()
                return held
            k, ms, per = (int(x) for x in a.child.split(","))
            t0 = time.perf_counter()
            ss.kmer_index(k, 20)
            t1 = time.perf_counter()
            out["index"] = ss.stats()
            cand = ss.prefilter(k, 20, min_shared=ms, min_per_1024=per)
            t2 = time.perf_counter()
            out["share"] = ss.stats()
            held = cand.hits(S, 11.0, 2.0, a.f_min)
            t3 = time.perf_counter()
            out["pass"] = ss.stats()
            out["wall_ms"], out["index_ms"], out["prefilter_ms"], out["hits_ms"] = 1e3 * (t3 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)
            out["candidates"] = len(cand)
            return held
        call()                                   # warm: code objects, buffers
        held = call()
        out["hits"] = len(held)
        np.savez(os.path.join(a.work, "hits_%s.npz" % a.child.replace(",", "_")), index=held.index, f=held.f)
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
        pairs = n * (n - 1) // 2
        cells = int((int(lens.sum()) ** 2 - int((lens ** 2).sum())) // 2)
        say("k-mer prefilter + Candidates.hits against SeqSet.hits on a resident sequence set")
        say("%d proteins in %d families of %d (ancestor of a C5 length, copies by workloads.mutate: substitutions %.2f, indels %.2f), %d residues"
            % (n, a.families, a.members, a.sub_rate, a.indel_rate, int(lens.sum())))
        say("upper block: %d pairs, %.4g cells; BLOSUM62 11 / 2 core local; %d alternating runs, a process each (warm call outside the timing)"
            % (pairs, cells, a.runs))
        if a.f_min is None:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "probe", "--work", work, "--members", str(a.members)],
                                 capture_output=True, text=True, timeout=900)
            got = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not got:
                say("the probe failed (exit %d): %s" % (out.returncode, (out.stdout + out.stderr)[-400:]))
                return 1
            pr = json.loads(got[0][7:])
            a.f_min = 0.5 * (pr["within_min"] + pr["across_max"])
            say("probe (SeqSet.score, every pair): f within a family min %.1f median %.1f; across families max %.1f median %.1f; %d failed pairs -> f_min %.1f%s"
                % (pr["within_min"], pr["within_median"], pr["across_max"], pr["across_median"], pr["failed"], a.f_min,
                   "" if pr["within_min"] > pr["across_max"] else " (the two ranges OVERLAP)"))
        res = {m: [] for m in MODES}
        for r in range(a.runs):
            for m in MODES:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", m, "--work", work, "--f-min", repr(a.f_min)],
                                     capture_output=True, text=True, timeout=900)
                got = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
                if out.returncode != 0 or not got:
                    say("run %d of %s failed (exit %d): %s" % (r, m, out.returncode, (out.stdout + out.stderr)[-400:]))
                    return 1
                res[m].append(json.loads(got[0][7:]))
        full = np.load(os.path.join(work, "hits_full.npz"))

        def med(v):
            return float(np.median(v))

        say()
        say("wall time per call [ms]: runs, median, spread (max - min)")
        walls = {}
        for m in MODES:
            w = [x["wall_ms"] for x in res[m]]
            walls[m] = w
            name = "SeqSet.hits (every pair)" if m == "full" else "kmer_index + prefilter + Candidates.hits, (k, min_shared, per 1024) = (%s)" % m.replace(",", ", ")
            say("%-82s %s  median %.1f  spread %.1f" % (name, " ".join("%.1f" % v for v in w), med(w), max(w) - min(w)))
        x = res["full"][-1]
        say()
        say("SeqSet.hits: %d hits; fill kernels %.1f ms, re-fill + walk %.1f ms, %.2f MB up, %.2f MB down"
            % (x["hits"], x["pass"]["fill_ms"], x["pass"]["refill_ms"], x["pass"]["bytes_up"] / 1e6, x["pass"]["bytes_down"] / 1e6))
        spread_full = max(walls["full"]) - min(walls["full"])
        for m in MODES[1:]:
            x = res[m][-1]
            got = np.load(os.path.join(work, "hits_%s.npz" % m.replace(",", "_")))
            common = np.isin(got["index"], full["index"])
            where = np.searchsorted(full["index"], got["index"][common])
            same_f = bool(common.all() and np.array_equal(got["f"].view(np.uint64), full["f"][where].view(np.uint64)))
            say()
            say("(%s): %d candidates of %d pairs (%.3f %%); %d hits, recall %d / %d = %.4f; every hit is a full hit with the same f bits: %s"
                % (m.replace(",", ", "), x["candidates"], pairs, 100.0 * x["candidates"] / pairs, x["hits"], int(common.sum()), len(full["index"]),
                   common.sum() / max(len(full["index"]), 1), same_f))
            say("  kmer_index: kernel %.3f ms, call %.1f ms; prefilter: sharing + compaction kernels %.3f ms, call %.1f ms, %.2f MB down"
                % (med([y["index"]["fetch_kernel_ms"] for y in res[m]]), med([y["index_ms"] for y in res[m]]),
                   med([y["share"]["fetch_kernel_ms"] for y in res[m]]), med([y["prefilter_ms"] for y in res[m]]), x["share"]["bytes_down"] / 1e6))
            say("  Candidates.hits: call %.1f ms; fill kernels %.1f ms, re-fill + walk %.1f ms, %.2f MB up, %.2f MB down"
                % (med([y["hits_ms"] for y in res[m]]), x["pass"]["fill_ms"], x["pass"]["refill_ms"], x["pass"]["bytes_up"] / 1e6, x["pass"]["bytes_down"] / 1e6))
            d = med(walls["full"]) - med(walls[m])
            half = 2 * x["candidates"] < pairs
            say("  against SeqSet.hits: %.1f ms %s at the median (SeqSet.hits' own spread: %.1f ms); fewer than half the pairs are candidates: %s -> criterion %s"
                % (abs(d), "less" if d > 0 else "MORE", spread_full, half, ("met" if d > spread_full else "MISSED") if half else "does not apply"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    if a.child:
        child()
    else:
        sys.exit(main())
