"""Identity filter of held hits: HeldHits.filter (aln_seqset_held_filter: every held hit's columns classed and counted on the
device, the kept positions compacted there, only they come down) against the path it replaces -- held.strings() on ALL hits
(48 + 2 * (N + M + 2) bytes per hit down) and the counting in numpy (tests/report_ref.py, the rule's restatement).
2 000 random proteins with C5's length distribution (those of tools/bench_allpairs.py), BLOSUM62 11 / 2 core local, `best` with
K = 10; min_identity 0.3, seed column skipped.  Both paths run in one session, alternating, three runs each: medians, spreads, bytes
both ways, and that both keep the same positions.
usage: python tools/bench_report.py [--n 2000] [--k 10] [--min-identity 0.3] [--runs 3] [--out profiles/r14_report.txt]"""
import argparse, os, sys, time
sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np
import report_ref
from aligner_amd import workloads
from aligner_amd.matrices import get_blosum62
from aligner_amd.seqset import SeqSet, rectangle

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2000)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--min-identity", type=float, default=0.3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default="profiles/r14_report.txt")
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
    ql, tl = lens[held.q], lens[held.t]
    say("Identity filter of held hits: HeldHits.filter against held.strings() on all hits + the numpy model")
    say("%d proteins (C5 lengths, %d residues), best K = %d: %d held; min_identity %.2f, seed column skipped; BLOSUM62 11 / 2 core local; %d runs each, alternating"
        % (n, int(lens.sum()), a.k, m, a.min_identity, a.runs))

    def new():
        pos, rep = held.filter(S, min_identity=a.min_identity, with_reports=True)
        return pos, ss.stats()

    def old():
        res, strings = held.strings()
        st = ss.stats()
        rep = report_ref.reports(strings, S, report_ref.SKIP_SEED, res["status"])
        return np.flatnonzero(report_ref.keep(rep, ql, tl, min_identity=a.min_identity)), st

    new(); old()                                             # warm: code objects, buffers
    t_new, t_old = [], []
    for r in range(a.runs):
        t0 = time.perf_counter(); pos_new, st_new = new(); t_new.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); pos_old, st_old = old(); t_old.append(time.perf_counter() - t0)

    def row(name, ts):
        say("%-58s %s  median %.1f  spread %.1f" % (name, " ".join("%.1f" % (1e3 * v) for v in ts), 1e3 * float(np.median(ts)), 1e3 * (max(ts) - min(ts))))

    say()
    say("wall time per call [ms]")
    row("HeldHits.filter (positions and reports of the kept)", t_new)
    row("baseline: held.strings() on all hits + numpy model", t_old)
    say()
    kept = len(pos_new)
    say("kept %d of %d hits; the two paths keep the same positions: %s" % (kept, m, "yes" if np.array_equal(pos_new, pos_old) else "NO"))
    say("HeldHits.filter: kernels %.3f ms, call %.3f ms; %.6f MB up, %.6f MB down (44 bytes per kept hit: %d)"
        % (st_new["fetch_kernel_ms"], st_new["wall_ms"], st_new["bytes_up"] / 1e6, st_new["bytes_down"] / 1e6, 44 * kept))
    derived = int((48 + 2 * (ql.astype(np.int64) + tl.astype(np.int64) + 2)).sum())
    say("baseline's fetch: kernels %.3f ms, call %.3f ms; %.6f MB up, %.6f MB down (48 + 2 (N + M + 2) per held hit: %d)"
        % (st_old["fetch_kernel_ms"], st_old["wall_ms"], st_old["bytes_up"] / 1e6, st_old["bytes_down"] / 1e6, derived))
    say("HeldHits.filter against the baseline: %.1f ms against %.1f ms (medians), %.1f x"
        % (1e3 * float(np.median(t_new)), 1e3 * float(np.median(t_old)), float(np.median(t_old)) / max(float(np.median(t_new)), 1e-9)))
    say("(the baseline's time is mostly the host's counting, hit by hit in numpy; its fetch alone is the `call` figure above)")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
