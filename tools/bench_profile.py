"""Profiles of a sequence set's families: HeldHits.profiles (aln_seqset_held_profiles: the held hits' columns counted on the device, one
integer matrix per family comes down) against the path that existed before -- held.strings() (48 + 2 (N + M + 2) bytes per hit down)
and the column loop of tests/profile_ref.py on the host.  The 2 000 proteins in 200 families of tools/bench_prefilter.py, prefiltered
with (k, min_shared, min_per_1024) = (3, 0, 256) on the full square, the 9 best candidates per record held (allpairs --kmer 3
--best-candidates 9), clustered greedily; seed column skipped, no filter.  Three alternating runs, a process each (set creation, the
held pass, the clustering and one warm call of the new path outside the timing); medians and spreads, the bytes both ways from
stats(), the summary, and that both paths give the same integers.
usage: python tools/bench_profile.py [--families 200] [--runs 3] [--out profiles/r18_profile.txt]"""
import argparse, json, os, subprocess, sys, tempfile, time
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
ap.add_argument("--out", default="profiles/r18_profile.txt")
ap.add_argument("--child", default=None, help="(internal) new | old")
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
    import profile_ref
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
        if a.child == "new":
            held.profiles(clusters)                  # warm: code object, buffers
            t0 = time.perf_counter()
            got = held.profiles(clusters)
            out["wall_ms"] = 1e3 * (time.perf_counter() - t0)
            out["stats"] = ss.stats()
            flat, records, out["summary"] = got.out, [tuple(int(x) for x in r) for r in got.records.tolist()], got.summary
        else:
            t0 = time.perf_counter()
            res, strs = held.strings()
            t1 = time.perf_counter()
            out["stats"] = ss.stats()
            flat, records, out["summary"] = profile_ref.profiles(held.q, held.t, res, strs, clusters.label.tolist(), centers, ss.len, ss.alphabet.volume(), 98, 1)
            t2 = time.perf_counter()
            out["wall_ms"], out["strings_ms"], out["loop_ms"] = 1e3 * (t2 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1)
        h = hashlib.sha256(np.ascontiguousarray(flat, dtype=np.uint32).tobytes())
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
        say("Profiles of a sequence set's families: HeldHits.profiles against held.strings() + the host's column loop")
        say("%d proteins in %d families of %d (ancestor of a C5 length, copies by workloads.mutate: substitutions %.2f, indels %.2f), %d residues"
            % (len(seqs), a.families, a.members, a.sub_rate, a.indel_rate, int(lens.sum())))
        say("prefilter (3, 0, 256) on the full square, the %d best candidates per record held, greedy clusters; BLOSUM62 11 / 2 core local; seed column skipped; %d alternating runs, a process each"
            % (a.best, a.runs))
        res = {m: [] for m in MODES}
        for r in range(a.runs):
            for m in MODES:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", m, "--work", work, "--best", str(a.best)],
                                     capture_output=True, text=True, timeout=900)
                got = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
                if out.returncode != 0 or not got:
                    say("run %d of %s failed (exit %d): %s" % (r, m, out.returncode, (out.stdout + out.stderr)[-400:]))
                    return 1
                res[m].append(json.loads(got[0][7:]))
        say()
        say("wall time per call [ms]: runs, median, spread (max - min)")
        for m, name in (("new", "HeldHits.profiles"), ("old", "baseline: held.strings() + the column loop of profile_ref")):
            w = [x["wall_ms"] for x in res[m]]
            say("%-62s %s  median %.1f  spread %.1f" % (name, " ".join("%.1f" % v for v in w), float(np.median(w)), max(w) - min(w)))
        x, y = res["new"][-1], res["old"][-1]
        say("baseline, last run: strings %.1f ms, loop %.1f ms" % (y["strings_ms"], y["loop_ms"]))
        say()
        say("%d held hits, %d families with a profile; summary %s" % (x["held"], x["families"], json.dumps(x["summary"])))
        say("HeldHits.profiles: kernels %.3f ms, call %.3f ms; %d bytes up, %d bytes down" % (x["stats"]["fetch_kernel_ms"], x["stats"]["wall_ms"],
                                                                                          x["stats"]["bytes_up"], x["stats"]["bytes_down"]))
        say("baseline: gather kernel %.3f ms, strings call %.3f ms; %d bytes up, %d bytes down" % (y["stats"]["fetch_kernel_ms"], y["stats"]["wall_ms"],
                                                                                                  y["stats"]["bytes_up"], y["stats"]["bytes_down"]))
        same = len({r["digest"] for m in MODES for r in res[m]}) == 1 and x["summary"] == y["summary"]
        say("both paths give the same elements, records and summary in every run: %s" % ("yes" if same else "NO"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    if a.child:
        child()
    else:
        sys.exit(main())
