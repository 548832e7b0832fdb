"""A stranded sequence set against a plain set of host-made 2n records, on one workload of nucleotide reads.

python tools/bench_strand.py [--reads N] [--length L] [--out profiles/r22_strand.txt]

Three things, each as the median of three alternating runs (plain, stranded, plain, ...) with the spread (max - min) and the bytes each
way: creating the set (the plain side pays for the reverse complements in numpy and uploads 2n records), one hits pass over the
both-strand rectangle q in [0, n) x t in [0, 2n), and the CIGARs of the held hits -- a stranded plan + fill against a plain plan + fill
plus the flip of coordinates and words in numpy.  The passes run the same kernels on the same bytes, so the expectation is that their
times sit inside the plain path's own spread and that the upload halves; the file says where that does not hold.  A record, not a gate.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from aligner_amd.enums import DNA  # noqa: E402
from aligner_amd.matrices import nucleotide_matrix  # noqa: E402
from aligner_amd.seqset import SeqSet, both, rectangle  # noqa: E402

DEL, EXT = 10.0, 1.0


def reads(n, length, seed=22):
    """n reads off a random genome of n * length / 4 residues (about four-fold cover), every other one from the opposite strand"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, size=max(n * length // 4, 2 * length)).astype(np.uint8)
    comp = DNA.complement_map()
    out = []
    for i in range(n):
        a = int(rng.integers(0, len(genome) - length))
        r = genome[a:a + int(length * (0.75 + 0.5 * rng.random()))].copy()
        flips = rng.random(len(r)) < 0.03
        r[flips] = (r[flips] + rng.integers(1, 4, size=int(flips.sum()))) % 4
        out.append(comp[r[::-1]] if i % 2 else r)
    return out


def flip_on_host(got, held, n, lengths):
    """what a caller of the plain plan does for PAF: coordinates onto the original records, the words of a mirrored target reversed"""
    rec = got.records.copy()
    qm, tm = held.q[got.which] >= n, held.t[got.which] >= n
    N, M = lengths[held.q[got.which]].astype(np.uint32), lengths[held.t[got.which]].astype(np.uint32)
    rec["q_start"], rec["q_end"] = np.where(qm, N - got.records["q_end"], got.records["q_start"]), np.where(qm, N - got.records["q_start"], got.records["q_end"])
    rec["t_start"], rec["t_end"] = np.where(tm, M - got.records["t_end"], got.records["t_start"]), np.where(tm, M - got.records["t_start"], got.records["t_end"])
    words = got.words.copy()
    for i in np.flatnonzero(tm):
        a, b = int(got.offsets[i]), int(got.offsets[i + 1])
        words[a:b] = got.words[a:b][::-1]
    return rec, words


def one(kind, recs, f_min):
    n = len(recs)
    m = nucleotide_matrix()
    out = {}
    t0 = time.perf_counter()
    if kind == "stranded":
        ss = SeqSet.stranded(recs, DNA)
    else:
        comp = DNA.complement_map()
        ss = SeqSet(recs + [comp[r[::-1]] for r in recs], DNA)
    out["create_ms"] = (time.perf_counter() - t0) * 1e3
    out["create_up"] = ss.stats()["bytes_up"]
    with ss:
        t0 = time.perf_counter()
        held = ss.hits(m, DEL, EXT, f_min, both(rectangle(0, n, 0, n), n))
        out["hits_ms"] = (time.perf_counter() - t0) * 1e3
        st = ss.stats()
        out["hits_fill_ms"], out["hits_up"], out["hits_down"], out["held"] = st["fill_ms"] + st["refill_ms"], st["bytes_up"], st["bytes_down"], len(held)
        t0 = time.perf_counter()
        if kind == "stranded":
            got = held.cigars(stranded=True)
            rec, words = got.records, got.words
        else:
            got = held.cigars()
            rec, words = flip_on_host(got, held, n, ss.len)
        out["cigar_ms"] = (time.perf_counter() - t0) * 1e3
        out["cigar_up"], out["cigar_down"] = held.last_cigar_plan_stats["bytes_up"], held.last_cigar_plan_stats["bytes_down"] + ss.stats()["bytes_down"]
        out["digest"] = (rec.tobytes(), words.tobytes(), held.f.tobytes())
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reads", type=int, default=300)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--f-min", type=float, default=1000.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    recs = reads(a.reads, a.length)
    one("stranded", recs[:8], a.f_min)                    # (warm: the library, the kernels, the context)
    runs = {"plain": [], "stranded": []}
    for _ in range(3):
        for kind in ("plain", "stranded"):
            runs[kind].append(one(kind, recs, a.f_min))
    same = all(r["digest"] == runs["plain"][0]["digest"] for k in runs for r in runs[k])
    lines = ["bench_strand: %d reads of about %d residues (%d residues), f_min %g, %d held hits; results %s" % (
        a.reads, a.length, sum(len(r) for r in recs), a.f_min, runs["plain"][0]["held"], "identical" if same else "DIFFER")]
    lines.append("%-10s %-9s %12s %12s %14s %14s" % ("step", "set", "median ms", "spread ms", "bytes up", "bytes down"))
    verdicts = []
    for step, up, down in (("create", "create_up", None), ("hits", "hits_up", "hits_down"), ("cigar", "cigar_up", "cigar_down")):
        stat = {}
        for kind in ("plain", "stranded"):
            v = sorted(r[step + "_ms"] for r in runs[kind])
            stat[kind] = (v[1], v[2] - v[0])
            lines.append("%-10s %-9s %12.3f %12.3f %14d %14s" % (step, kind, v[1], v[2] - v[0], runs[kind][0][up], runs[kind][0][down] if down else "-"))
        inside = abs(stat["stranded"][0] - stat["plain"][0]) <= stat["plain"][1]
        verdicts.append("%s: stranded median %s the plain path's spread (%.3f vs %.3f +- %.3f ms)" % (
            step, "inside" if inside else "OUTSIDE", stat["stranded"][0], stat["plain"][0], stat["plain"][1]))
    lines += verdicts
    lines.append("upload at creation: stranded %d bytes, plain %d bytes (%.2f x)" % (
        runs["stranded"][0]["create_up"], runs["plain"][0]["create_up"], runs["plain"][0]["create_up"] / max(runs["stranded"][0]["create_up"], 1)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
