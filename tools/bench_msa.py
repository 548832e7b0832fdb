"""Family alignments of a sequence set: HeldHits.msa (aln_seqset_held_msa_plan + _fill: inserts measured, columns laid out and rows written
on the device; the matrices and row lists come down) against the path that existed before -- held.strings() (48 + 2 (N + M + 2) bytes
per hit down) and the centre-star merge of tests/msa_ref.py on the host.  The set of tools/bench_prefilter.py and tools/bench_profile.py:
2 000 proteins in 200 families, prefiltered with (k, min_shared, min_per_1024) = (3, 0, 256) on the full square, the 9 best candidates
per record held, clustered greedily; no filter.  Three alternating runs, a process each (set creation, the held pass, the clustering
and one warm call of the new path outside the timing); medians and spreads, the bytes both ways from stats(), the summary, and that
both paths give the same bytes.  Then one run of the new path under `rocprofv3 --kernel-trace --stats`, a process of its own, for the
share of the rank kernel (O(rows^2) per family) among the call's kernels.
usage: python tools/bench_msa.py [--families 200] [--runs 3] [--out profiles/r19_msa.txt] [--no-trace]"""
import argparse, csv, glob, json, os, subprocess, sys, tempfile, time
sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--families", type=int, default=200)
ap.add_argument("--members", type=int, default=10)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--best", type=int, default=9)
ap.add_argument("--sub-rate", type=float, default=0.15)
ap.add_argument("--indel-rate", type=float, default=0.02)
ap.add_argument("--out", default="profiles/r19_msa.txt")
ap.add_argument("--no-trace", action="store_true", help="leave out the run under rocprofv3")
ap.add_argument("--child", default=None, help="(internal) new | old | trace")
ap.add_argument("--work", default=None, help="(internal) the workload and result files' directory")
a = ap.parse_args()
MODES = ["new", "old"]


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
    import hashlib
    import msa_ref
    from aligner_amd import profile
    from aligner_amd.matrices import get_blosum62
    from aligner_amd.seqset import SeqSet, rectangle
    data = np.load(os.path.join(a.work, "workload.npz"))
    seqs = np.split(data["residues"], np.cumsum(data["lens"])[:-1])
    S = get_blosum62()
    out = {"mode": a.child}
    with SeqSet(seqs) as ss:
        n = len(ss)
        cand = ss.prefilter(3, 20, min_shared=0, min_per_1024=256, block=rectangle(0, n, 0, n))
        held = cand.best(S, 11.0, 2.0, a.best, skip_self=True)
        clusters = held.cluster(mode="greedy")
        centers = profile.default_centers(clusters.label)
        out["held"], out["families"] = len(held), len(centers)
        if a.child in ("new", "trace"):
            held.msa(clusters)                       # warm: code object, buffers
            t0 = time.perf_counter()
            got = held.msa(clusters)
            out["wall_ms"] = 1e3 * (time.perf_counter() - t0)
            out["plan"], out["fill"] = held.last_msa_plan_stats, ss.stats()
            flat, rows, records, out["summary"] = got.out, got.row_hit, [tuple(int(x) for x in r) for r in got.records.tolist()], got.summary
        else:
            t0 = time.perf_counter()
            res, strs = held.strings()
            t1 = time.perf_counter()
            out["stats"] = ss.stats()
            own = [ss.seqs[int(o):int(o) + int(l)] for o, l in zip(ss.off, ss.len)]
            mats, lists, records, out["summary"] = msa_ref.alignments(held.q, held.t, res, strs, clusters.label.tolist(), centers, ss.len, own, 98)
            flat, rows = msa_ref.flat(mats, lists)
            t2 = time.perf_counter()
            out["wall_ms"], out["strings_ms"], out["merge_ms"] = 1e3 * (t2 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1)
        h = hashlib.sha256(np.ascontiguousarray(flat, dtype=np.uint8).tobytes())
        h.update(np.ascontiguousarray(rows, dtype=np.uint32).tobytes())
        h.update(repr(records).encode())
        out["digest"] = h.hexdigest()
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
        say("Family alignments of a sequence set: HeldHits.msa against held.strings() + the host's centre-star merge")
        say("%d proteins in %d families of %d (ancestor of a C5 length, copies by workloads.mutate: substitutions %.2f, indels %.2f), %d residues"
            % (len(seqs), a.families, a.members, a.sub_rate, a.indel_rate, int(lens.sum())))
        say("prefilter (3, 0, 256) on the full square, the %d best candidates per record held, greedy clusters; BLOSUM62 11 / 2 core local; no filter; %d alternating runs, a process each"
            % (a.best, a.runs))
        me = [sys.executable, os.path.abspath(__file__), "--work", work, "--best", str(a.best)]
        res = {m: [] for m in MODES}
        for r in range(a.runs):
            for m in MODES:
                out = subprocess.run(me + ["--child", m], capture_output=True, text=True, timeout=900)
                got = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
                if out.returncode != 0 or not got:
                    say("run %d of %s failed (exit %d): %s" % (r, m, out.returncode, (out.stdout + out.stderr)[-400:]))
                    return 1
                res[m].append(json.loads(got[0][7:]))
        say()
        say("wall time per call [ms]: runs, median, spread (max - min)")
        for m, name in (("new", "HeldHits.msa (plan + fill)"), ("old", "baseline: held.strings() + the merge of msa_ref")):
            w = [x["wall_ms"] for x in res[m]]
            say("%-62s %s  median %.1f  spread %.1f" % (name, " ".join("%.1f" % v for v in w), float(np.median(w)), max(w) - min(w)))
        x, y = res["new"][-1], res["old"][-1]
        say("baseline, last run: strings %.1f ms, merge %.1f ms" % (y["strings_ms"], y["merge_ms"]))
        say()
        say("%d held hits, %d families; summary %s" % (x["held"], x["families"], json.dumps(x["summary"])))
        say("plan: kernels %.3f ms, call %.3f ms; %d bytes up, %d bytes down" % (x["plan"]["fetch_kernel_ms"], x["plan"]["wall_ms"], x["plan"]["bytes_up"],
                                                                                x["plan"]["bytes_down"]))
        say("fill: kernels %.3f ms, call %.3f ms; %d bytes up, %d bytes down" % (x["fill"]["fetch_kernel_ms"], x["fill"]["wall_ms"], x["fill"]["bytes_up"],
                                                                                x["fill"]["bytes_down"]))
        say("baseline: gather kernel %.3f ms, strings call %.3f ms; %d bytes up, %d bytes down" % (y["stats"]["fetch_kernel_ms"], y["stats"]["wall_ms"],
                                                                                                  y["stats"]["bytes_up"], y["stats"]["bytes_down"]))
        same = len({r["digest"] for m in MODES for r in res[m]}) == 1 and x["summary"] == y["summary"]
        say("both paths give the same matrices, row lists, records and summary in every run: %s" % ("yes" if same else "NO"))
        if not a.no_trace:
            say()
            trace = os.path.join(work, "trace")
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "--"] + me + ["--child", "trace"]
            try:
                rc = subprocess.call(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
            except (subprocess.TimeoutExpired, OSError):
                rc = 124
            mine = {}
            for path in sorted(glob.glob(os.path.join(trace, "**", "*kernel_stats.csv"), recursive=True)):
                for rec in csv.DictReader(open(path)):
                    name = rec.get("Name", "")
                    if name.startswith("aln_msa_"):
                        calls = int(rec.get("Calls") or 0)
                        mine[name.split("(")[0]] = (calls, float(rec.get("TotalDurationNs") or calls * float(rec.get("AverageNs") or 0)))
            if rc != 0 or not mine:
                say("the run under rocprofv3 gave no kernel statistics (exit %d): the rank kernel's share is not measured" % rc)
            else:
                total = sum(ns for _c, ns in mine.values())
                say("rocprofv3 --kernel-trace --stats, a run of its own (two calls of HeldHits.msa): the call's kernels")
                for name, (calls, ns) in sorted(mine.items()):
                    say("  %-28s calls %3d  total %10.1f us  %5.1f %%" % (name, calls, ns / 1e3, 100.0 * ns / total))
                rank = mine.get("aln_msa_rank_kernel", (0, 0.0))[1]
                say("share of the rank kernel among the kernels of plan + fill: %.1f %%" % (100.0 * rank / total))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    if a.child:
        child()
    else:
        sys.exit(main())
