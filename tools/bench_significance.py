"""Significance of held hits: HeldHits.significance (aln_seqset_held_significance: copies drawn from the resident residues, one
48-byte record per hit reduced on the device) against this tree's path over the same hits without it -- held_list, then
statistics.device_shuffled_scores on the listed pairs (their residues uploaded again, 8 bytes per copy down), then numpy moments.
2 000 random proteins with C5's length distribution, BLOSUM62 11 / 2 core local, `best` with K = 10; significance of 2 000 of the
hits at 4 999 copies.  Both paths run in one session, alternating, three runs each: medians, spreads, bytes both ways.  Both run
the same fill, so no speed-up is expected; the claim to check is the bytes, and that the new call is not slower beyond the
baseline's own spread.
usage: python tools/bench_significance.py [--n 2000] [--k 10] [--hits 2000] [--copies 4999] [--runs 3] [--out profiles/r13_significance.txt]"""
import argparse, os, sys, time
sys.path.insert(0, ".")
import numpy as np
from aligner_amd import statistics, workloads
from aligner_amd.batch import PairBatch
from aligner_amd.matrices import get_blosum62
from aligner_amd.seqset import SeqSet, rectangle

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2000)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--hits", type=int, default=2000)
ap.add_argument("--copies", type=int, default=4999)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--seed", type=int, default=13)
ap.add_argument("--out", default="profiles/r13_significance.txt")
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
    keep = np.linspace(0, len(held) - 1, min(a.hits, len(held))).astype(np.uint32)        # spread over the queries
    m = len(keep)
    cells = float((lens[held.q[keep]].astype(np.float64) * lens[held.t[keep]].astype(np.float64)).sum()) * a.copies
    say("Significance of held hits: HeldHits.significance against held_list + device_shuffled_scores + numpy moments")
    say("%d proteins (C5 lengths, %d residues), best K = %d: %d held; %d of them at %d copies: about %.4g cells; BLOSUM62 11 / 2 core local; %d runs each, alternating"
        % (n, int(lens.sum()), a.k, len(held), m, a.copies, cells, a.runs))

    def new():
        sig = held.significance(S, 11.0, 2.0, a.seed, per_pair=a.copies, keep=keep)
        return sig, ss.stats()

    def old():
        q, t = held.q[keep], held.t[keep]                   # (held_list: the host's list)
        b = PairBatch(residues, off[q], lens[q].astype(np.uint64), off[t], lens[t].astype(np.uint64))
        # one call over the listed pairs; their streams are then (seed, position): other copies than the new call's, the same work
        f, L, st = statistics.device_shuffled_scores(b, 11.0, 2.0, S, a.seed, per_pair=a.copies, check=False)
        mean = f.mean(axis=1)
        sd = np.sqrt(np.maximum((f * f).mean(axis=1) - mean * mean, 0.0))
        with np.errstate(all="ignore"):
            z = (held.f[keep] - mean) / sd
        p = ((f >= held.f[keep][:, None]).sum(axis=1) + 1.0) / (a.copies + 1.0)
        # aln_shuffle_scores reports no byte counts: these two are DERIVED here from what it moves -- up: the residues as its staging
        # sends them (one span of the caller's buffer if that is at most twice the listed residues + 64 KiB, the listed ranges packed
        # otherwise) and the 32-byte pair table; down: 8 bytes per copy and 4 per pair
        lo = int(min(off[q].min(), off[t].min()))
        hi = int(max((off[q] + lens[q]).max(), (off[t] + lens[t]).max()))
        listed = int(lens[q].sum() + lens[t].sum())
        span = hi - lo if hi - lo <= 2 * listed + 65536 else listed
        return (z, p), dict(bytes_up=span + 32 * m, bytes_down=8 * m * a.copies + 4 * m)

    new(); old()                                             # warm: code objects, buffers
    t_new, t_old, st_new, st_old = [], [], None, None
    for r in range(a.runs):
        t0 = time.perf_counter(); sig, st_new = new(); t_new.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); zp, st_old = old(); t_old.append(time.perf_counter() - t0)

    def row(name, ts):
        say("%-58s %s  median %.1f  spread %.1f" % (name, " ".join("%.1f" % (1e3 * v) for v in ts), 1e3 * float(np.median(ts)), 1e3 * (max(ts) - min(ts))))

    say()
    say("wall time per call [ms]")
    row("HeldHits.significance", t_new)
    row("baseline: device_shuffled_scores + numpy moments", t_old)
    say()
    say("HeldHits.significance: kernels %.1f ms; %.3f MB up, %.3f MB down (%.0f bytes per hit)"
        % (st_new["fetch_kernel_ms"], st_new["bytes_up"] / 1e6, st_new["bytes_down"] / 1e6, st_new["bytes_down"] / m))
    say("baseline (derived, not reported by the library): %.3f MB up (residues and pair table), %.3f MB down (%.0f bytes per hit)"
        % (st_old["bytes_up"] / 1e6, st_old["bytes_down"] / 1e6, st_old["bytes_down"] / m))
    say("z of the two (other streams: the same distribution, not the same copies): median |dz| %.3f; hits with p_emp <= 0.001: %d and %d of %d"
        % (float(np.nanmedian(np.abs(sig["z"] - zp[0]))), int((sig["p_emp"] <= 0.001).sum()), int((zp[1] <= 0.001).sum()), m))
    d = float(np.median(t_new) - np.median(t_old))
    noise = max(t_old) - min(t_old)
    say("HeldHits.significance against the baseline: %.1f ms %s (the baseline's own spread: %.1f ms)%s"
        % (1e3 * abs(d), "MORE" if d > 0 else "less", 1e3 * noise, " -- slower beyond the spread" if d > noise else ""))
    say("(the two sides draw other streams, so their copies' trims differ: the same cells in expectation, not copy by copy -- a difference")
    say(" within the spread says nothing either way)")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
