"""CIGARs of a sequence set's held hits: HeldHits.cigars (aln_seqset_held_cigar_plan + _fill: runs counted, offsets scanned and words
written on the device; 32 bytes per hit, the words and the offsets come down) against the path that existed before -- held.strings()
(48 + 2 (N + M + 2) bytes per hit down) and cigar.encode on the host, hit by hit.  The set of tools/bench_profile.py and
tools/bench_msa.py: 2 000 proteins in 200 families, prefiltered with (k, min_shared, min_per_1024) = (3, 0, 256) on the full square,
the 9 best candidates per record held.  Three alternating runs, a process each (set creation, the held pass and one warm call of the new
path outside the timing); medians and spreads, the bytes both ways from stats(), the summary, and that both paths give the same words.
usage: python tools/bench_cigar.py [--families 200] [--runs 3] [--eqx] [--out profiles/r20_cigar.txt]"""
import argparse, json, os, subprocess, sys, tempfile, time
sys.path.insert(0, ".")
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--families", type=int, default=200)
ap.add_argument("--members", type=int, default=10)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--best", type=int, default=9)
ap.add_argument("--sub-rate", type=float, default=0.15)
ap.add_argument("--indel-rate", type=float, default=0.02)
ap.add_argument("--eqx", action="store_true", help="= and X in place of M, on both paths")
ap.add_argument("--out", default="profiles/r20_cigar.txt")
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
    from aligner_amd import cigar
    from aligner_amd.matrices import get_blosum62
    from aligner_amd.seqset import SeqSet, rectangle
    data = np.load(os.path.join(a.work, "workload.npz"))
    seqs = np.split(data["residues"], np.cumsum(data["lens"])[:-1])
    S = get_blosum62()
    flags = cigar.EXTENDED if a.eqx else 0
    out = {"mode": a.child}
    with SeqSet(seqs) as ss:
        n = len(ss)
        cand = ss.prefilter(3, 20, min_shared=0, min_per_1024=256, block=rectangle(0, n, 0, n))
        held = cand.best(S, 11.0, 2.0, a.best, skip_self=True)
        out["held"] = len(held)
        if a.child == "new":
            held.cigars(extended=a.eqx)              # warm: code object, buffers
            t0 = time.perf_counter()
            got = held.cigars(extended=a.eqx)
            out["wall_ms"] = 1e3 * (time.perf_counter() - t0)
            out["plan"], out["fill"] = held.last_cigar_plan_stats, ss.stats()
            words, records, out["summary"] = got.words, got.records, got.summary
        else:
            t0 = time.perf_counter()
            res, strs = held.strings()
            t1 = time.perf_counter()
            out["stats"] = ss.stats()
            records = np.zeros(len(held), dtype=cigar.RECORD_DTYPE)
            parts, padded, overflow = [], 0, 0
            for h in range(len(held)):
                rec, w, p, o = cigar.encode(strs[h][0], strs[h][1], 98, flags, int(res["start_x"][h]), int(res["start_y"][h]), int(ss.len[held.q[h]]),
                                            int(res["status"][h]))
                records[h] = rec
                parts.append(w)
                padded += p
                overflow += o
            words = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
            t2 = time.perf_counter()
            out["summary"] = dict(held=len(held), listed=len(held), total_ops=int(len(words)), failed=int((records["status"] != 0).sum()), padded=padded,
                                  overflow=overflow)
            out["wall_ms"], out["strings_ms"], out["encode_ms"] = 1e3 * (t2 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1)
        h = hashlib.sha256(np.ascontiguousarray(words, dtype=np.uint32).tobytes())
        h.update(np.ascontiguousarray(records).tobytes())
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
        say("CIGARs of a sequence set's held hits: HeldHits.cigars against held.strings() + cigar.encode on the host")
        say("%d proteins in %d families of %d (ancestor of a C5 length, copies by workloads.mutate: substitutions %.2f, indels %.2f), %d residues"
            % (len(seqs), a.families, a.members, a.sub_rate, a.indel_rate, int(lens.sum())))
        say("prefilter (3, 0, 256) on the full square, the %d best candidates per record held; BLOSUM62 11 / 2 core local; ops %s; %d alternating runs, a process each"
            % (a.best, "= X I D" if a.eqx else "M I D", a.runs))
        me = [sys.executable, os.path.abspath(__file__), "--work", work, "--best", str(a.best)] + (["--eqx"] if a.eqx else [])
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
        for m, name in (("new", "HeldHits.cigars (plan + fill)"), ("old", "baseline: held.strings() + cigar.encode per hit")):
            w = [x["wall_ms"] for x in res[m]]
            say("%-62s %s  median %.1f  spread %.1f" % (name, " ".join("%.1f" % v for v in w), float(np.median(w)), max(w) - min(w)))
        s = [x["strings_ms"] for x in res["old"]]
        say("%-62s %s  median %.1f  spread %.1f" % ("baseline, held.strings() alone (the rest is a Python loop)", " ".join("%.1f" % v for v in s),
                                                    float(np.median(s)), max(s) - min(s)))
        x, y = res["new"][-1], res["old"][-1]
        say()
        say("%d held hits; summary %s" % (x["held"], json.dumps(x["summary"])))
        say("plan: kernels %.3f ms, call %.3f ms; %d bytes up, %d bytes down" % (x["plan"]["fetch_kernel_ms"], x["plan"]["wall_ms"], x["plan"]["bytes_up"],
                                                                                x["plan"]["bytes_down"]))
        say("fill: kernels %.3f ms, call %.3f ms; %d bytes up, %d bytes down" % (x["fill"]["fetch_kernel_ms"], x["fill"]["wall_ms"], x["fill"]["bytes_up"],
                                                                                x["fill"]["bytes_down"]))
        say("baseline: gather kernel %.3f ms, strings call %.3f ms; %d bytes up, %d bytes down" % (y["stats"]["fetch_kernel_ms"], y["stats"]["wall_ms"],
                                                                                                  y["stats"]["bytes_up"], y["stats"]["bytes_down"]))
        down = x["plan"]["bytes_down"] + x["fill"]["bytes_down"]
        say("bytes down per held hit: %.1f against %.1f" % (down / max(x["held"], 1), y["stats"]["bytes_down"] / max(x["held"], 1)))
        same = len({r["digest"] for m in MODES for r in res[m]}) == 1 and all(r["summary"] == x["summary"] for m in MODES for r in res[m])
        say("both paths give the same words, records and summary in every run: %s" % ("yes" if same else "NO"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    if a.child:
        child()
    else:
        sys.exit(main())
