"""The sorted word index and its join against the bitmap route of the prefilter, on the family set of tools/bench_prefilter.py (2 000
proteins in 200 families of 10, C5 lengths, substitution rate 0.15, indel rate 0.02) and on a set ten times as large made by the same
generator (--scale 10: 2 000 families).
  (4, 8, 128)      SeqSet.word_index + word_join against SeqSet.kmer_index + prefilter on the upper block, the two lists asserted equal
  k = 5, k = 6     the join alone (min_shared 2, min_per_1024 0): candidates, and recall against the within-family pairs
Three alternating runs of every case in one process after one warm call of each kind; per case the median and the spread (max - min)
of the wall time and of the kernels' time, index and join apart, and the bytes that came down (aln_seqset_stats).
usage: python tools/bench_wordjoin.py [--families 200] [--scale 1,10] [--runs 3] [--out profiles/r21_wordjoin.txt]"""
import argparse, os, sys, time
sys.path.insert(0, ".")
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--families", type=int, default=200)
ap.add_argument("--members", type=int, default=10)
ap.add_argument("--scale", default="1,10")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--sub-rate", type=float, default=0.15)
ap.add_argument("--indel-rate", type=float, default=0.02)
ap.add_argument("--out", default="profiles/r21_wordjoin.txt")
a = ap.parse_args()


def workload(families):
    from aligner_amd import workloads
    lens = workloads.c5_lengths(families)[0]
    seqs = []
    for fam in range(families):
        anc = workloads.random_codes(workloads.SEED_C5 + 1000 + fam, int(lens[fam]), 20)
        seqs.append(anc)
        for m in range(1, a.members):
            seqs.append(np.asarray(workloads.mutate(anc, workloads.SEED_C5 + 100000 + fam * 64 + m, 20, a.sub_rate, a.indel_rate), dtype=np.uint8))
    return seqs


def timed(ss, call):
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    st = ss.stats()
    return out, wall, st["fetch_kernel_ms"], st["bytes_down"]


def summary(rows):
    """rows: per run (wall, kernels, bytes) -> median and spread of the first two, the bytes of the last run"""
    w, k = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    return "wall %.2f ms (spread %.2f), kernels %.2f ms (spread %.2f), %d bytes down" % (np.median(w), w.max() - w.min(), np.median(k), k.max() - k.min(), rows[-1][2])


def main():
    from aligner_amd.seqset import SeqSet
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("tools/bench_wordjoin.py: word_index + word_join against kmer_index + prefilter; %d alternating runs, median (spread)" % a.runs)
    for scale in [int(x) for x in a.scale.split(",")]:
        families = a.families * scale
        seqs = workload(families)
        n = len(seqs)
        fam = np.arange(n) // a.members
        within = families * a.members * (a.members - 1) // 2
        say()
        say("%d proteins in %d families of %d, %d residues, %d pairs, %d within families" % (n, families, a.members, sum(len(s) for s in seqs), n * (n - 1) // 2, within))
        with SeqSet(seqs) as ss:
            k, ms, per = 4, 8, 128
            cases = {"bitmaps": (lambda: ss.kmer_index(k, 20), lambda: ss.prefilter(k, 20, min_shared=ms, min_per_1024=per)),
                     "join": (lambda: ss.word_index(k, 20), lambda: ss.word_join(k, 20, min_shared=ms, min_per_1024=per))}
            for index, run in cases.values():                                    # warm
                index(); run()
            got = {name: dict(index=[], run=[]) for name in cases}
            lists = {}
            for _ in range(a.runs):
                for name, (index, run) in cases.items():
                    _, w, kk, by = timed(ss, index)
                    got[name]["index"].append((w, kk, by))
                    cand, w, kk, by = timed(ss, run)
                    got[name]["run"].append((w, kk, by))
                    lists[name] = cand
            x, y = lists["bitmaps"], lists["join"]
            assert len(x) == len(y) and (x.index == y.index).all() and (x.q == y.q).all() and (x.t == y.t).all() and (x.shared == y.shared).all()
            say("(4, 8, 128): %d candidates by both routes, lists equal" % len(x))
            for name in cases:
                say("  %-8s index %s" % (name, summary(got[name]["index"])))
                say("  %-8s pairs %s" % (name, summary(got[name]["run"])))
                tot = np.array([i[0] + r[0] for i, r in zip(got[name]["index"], got[name]["run"])])
                say("  %-8s index + pairs: wall %.2f ms (spread %.2f)" % (name, np.median(tot), tot.max() - tot.min()))
            for k in (5, 6):
                ss.word_index(k, 20); ss.word_join(k, 20, min_shared=2)
                rows_i, rows_j = [], []
                for _ in range(a.runs):
                    _, w, kk, by = timed(ss, lambda: ss.word_index(k, 20))
                    rows_i.append((w, kk, by))
                    cand, w, kk, by = timed(ss, lambda: ss.word_join(k, 20, min_shared=2))
                    rows_j.append((w, kk, by))
                hit = int((fam[cand.q] == fam[cand.t]).sum())
                say("k = %d, min_shared 2: %d candidates, %d of the %d within-family pairs (recall %.4f)" % (k, len(cand), hit, within, hit / within))
                say("  join     index %s" % summary(rows_i))
                say("  join     pairs %s" % summary(rows_j))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
