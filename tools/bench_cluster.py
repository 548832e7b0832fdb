"""Clustering a sequence set by its held hits: HeldHits.cluster (aln_seqset_held_cluster: the hits filtered, grouped and listed on
the device; 4 bytes per sequence and 16 per cluster come down) against what a caller did before -- HeldHits.filter (44 bytes per
kept hit down), held_list (24 bytes per held hit) and a union-find or a greedy pass on the host (tests/cluster_ref.py).
2 000 random proteins with C5's length distribution (the setup of tools/bench_report.py), BLOSUM62 11 / 2 core local, `best` with
K = 10; min_identity 0.3, seed column skipped; both modes.  Both paths run in one session, alternating, three runs each: medians,
spreads, bytes both ways, and that both give the same labels.
usage: python tools/bench_cluster.py [--n 2000] [--k 10] [--min-identity 0.3] [--runs 3] [--out profiles/r15_cluster.txt]"""
import argparse, os, sys, time
sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np
import cluster_ref
from aligner_amd import workloads
from aligner_amd.matrices import get_blosum62
from aligner_amd.seqset import HeldHits, SeqSet, rectangle

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2000)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--min-identity", type=float, default=0.3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default="profiles/r15_cluster.txt")
a = ap.parse_args()

n = a.n
lens = workloads.c5_lengths(n)[0]
off = np.zeros(n, dtype=np.uint64)
off[1:] = np.cumsum(lens)[:-1]
residues = workloads.random_codes(workloads.SEED_C5 + 7, int(lens.sum()), 20)
seqs = [residues[int(o):int(o) + int(l)] for o, l in zip(off, lens)]
S = get_blosum62()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


with SeqSet(seqs) as ss:
    held = ss.best(S, 11.0, 2.0, a.k, block=rectangle(0, n, 0, n), skip_self=True)
    m = len(held)
    say("Clusters of a sequence set by its held hits: HeldHits.cluster against filter + held_list + the host's pass")
    say("%d proteins (C5 lengths, %d residues), best K = %d: %d held; min_identity %.2f, seed column skipped; BLOSUM62 11 / 2 core local; %d runs each, alternating"
        % (n, int(lens.sum()), a.k, m, a.min_identity, a.runs))
    for name, mode in (("components", cluster_ref.COMPONENTS), ("greedy", cluster_ref.GREEDY)):

        def new():
            got = held.cluster(S, mode=name, min_identity=a.min_identity)
            return got, ss.stats()

        def old():
            pos, rep = held.filter(S, min_identity=a.min_identity, with_reports=True)
            st = ss.stats()
            lst = HeldHits(ss, m, held.semantics)                  # held_list: 24 bytes per held hit
            lab = cluster_ref.labels(mode, n, lst.q[pos].tolist(), lst.t[pos].tolist(), lens.tolist())
            return np.array(lab, dtype=np.uint32), st, len(pos)

        new(); old()                                             # warm: code objects, buffers
        t_new, t_old = [], []
        for r in range(a.runs):
            t0 = time.perf_counter(); got, st_new = new(); t_new.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); lab_old, st_old, kept = old(); t_old.append(time.perf_counter() - t0)

        def row(what, ts):
            say("%-58s %s  median %.1f  spread %.1f" % (what, " ".join("%.1f" % (1e3 * v) for v in ts), 1e3 * float(np.median(ts)), 1e3 * (max(ts) - min(ts))))

        say()
        say("mode %s: wall time per call [ms]" % name)
        row("HeldHits.cluster", t_new)
        row("baseline: filter + held_list + the host's pass", t_old)
        s = got.summary
        say("%d edges of %d hits; %d clusters, %d singletons, %d rounds; the two paths give the same labels: %s"
            % (s["edges"] + s["self_edges"], m, s["clusters"], s["singletons"], s["rounds"], "yes" if np.array_equal(got.label, lab_old) else "NO"))
        say("HeldHits.cluster: kernels %.3f ms, call %.3f ms; %d bytes up, %d bytes down (4 per sequence + 16 per cluster + 32 + 4 per round: %d)"
            % (st_new["fetch_kernel_ms"], st_new["wall_ms"], st_new["bytes_up"], st_new["bytes_down"], 4 * n + 16 * s["clusters"] + 32 + 4 * s["rounds"]))
        say("baseline: filter's kernels %.3f ms, call %.3f ms; %d bytes up, %d bytes down from the filter (44 per kept hit: %d) and %d from held_list (24 per held hit)"
            % (st_old["fetch_kernel_ms"], st_old["wall_ms"], st_old["bytes_up"], st_old["bytes_down"], 44 * kept, 24 * m))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
