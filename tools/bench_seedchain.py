"""Seed chains against the fill as the way to learn where an overlap lies, on the reads of tools/bench_seedjoin.py (same generator, same
seeds, both strands), k = 15, with max_occ 40 and 0.

(a) chain: seed_join (threshold 1, bench_seedjoin's band) + chain_filter at the largest min_score that loses none of the true overlaps
    the join lists (the least chain score over them, found by a first `chains` call in the same process, which also warms the kernels):
    candidates kept, recall against the planted overlaps, kernels and wall of join and filter, bytes down.
(b) hits: what a caller does today for the same information: seed_join at bench_seedjoin's threshold (the least seeds over the true
    overlaps listed) + Candidates.hits at the benchmark's f_min, then the held hits' start and end cells (the CIGAR records).
(c) how far q_start .. q_end / t_start .. t_end of (a) lie from the aligned region of (b), over the pairs both hold, as a distribution
    of absolute differences, the planted overlaps and the other pairs apart (computed in the `hits` child, which runs the chains once
    more, untimed).

Every (route, run) is a process of its own (--child); the routes alternate, --runs times; the medians and spreads go to --out.
usage: python tools/bench_seedchain.py [--runs 3] [--out profiles/r27_seedchain.txt]"""
import argparse, importlib.util, json, os, subprocess, sys, time
sys.path.insert(0, ".")
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--k", type=int, default=15)
ap.add_argument("--max-gap", type=int, default=1000)
ap.add_argument("--max-skew", type=int, default=200)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default="profiles/r27_seedchain.txt")
ap.add_argument("--child", default=None, help="one route in this process: chain40, hits40, chain0, hits0; prints one JSON line")
a = ap.parse_args()
ROUTES = ["chain40", "hits40", "chain0", "hits0"]            # the number: max_occ


def seedjoin_bench():
    """tools/bench_seedjoin.py as a module, under its own defaults: its workload() is the generator"""
    argv, sys.argv = sys.argv, [sys.argv[0]]
    try:
        spec = importlib.util.spec_from_file_location("bench_seedjoin", os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_seedjoin.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.argv = argv
    return mod


def at_true(index, true_pair):
    """(where each true pair stands in the ascending list `index`, whether it is listed)"""
    at = np.searchsorted(index, true_pair)
    at[at >= len(index)] = 0
    return at, (index[at].astype(np.int64) == true_pair if len(index) else np.zeros(len(true_pair), dtype=bool))


def child(route):
    from aligner_amd.enums import DNA
    from aligner_amd.matrices import nucleotide_matrix
    from aligner_amd.seqset import SeqSet, both, rectangle
    bj = seedjoin_bench()
    reads, tq, tt, _text = bj.workload()
    n = len(reads)
    true_pair = np.sort(tq * (2 * n) + tt)
    max_occ = int(route[5 if route.startswith("chain") else 4:])
    kw = dict(max_gap=a.max_gap, max_skew=a.max_skew, max_occ=max_occ)
    with SeqSet.stranded(reads, DNA) as ss:
        block = both(rectangle(0, n, 0, n), n)
        ss.seed_index(a.k, 4)
        join = lambda least: ss.seed_join(a.k, 4, min_seeds=least, band=bj.a.band, max_occ=max_occ, block=block)
        loose = join(1)
        at, listed = at_true(loose.index, true_pair)
        recs = loose.chains(**kw)                                                # the warm call of the chain kernels, and the thresholds
        chained = listed & (recs["flags"][at] == 0)
        least_score = int(recs["score"][at[chained]].min()) if chained.any() else 0
        least_seeds = int(loose.shared[at[listed]].min()) if listed.any() else 1
        out = dict(route=route, true=len(true_pair), listed_at_1=int(listed.sum()), at_threshold_1=len(loose), chain_summary=loose.chain_summary)
        if route.startswith("chain"):
            cand, jw, jk, jb = bj.timed(ss, lambda: join(1))
            kept, fw, fk, fb = bj.timed(ss, lambda: cand.chain_filter(least_score, 0, **kw))
            out.update(min_score=least_score, candidates=len(kept), kept=int(np.isin(true_pair, kept.index.astype(np.int64)).sum()),
                       overflowed=kept.summary["overflowed"], join_wall=jw, join_kernels=jk, join_bytes=jb, filter_wall=fw, filter_kernels=fk, filter_bytes=fb,
                       wall=jw + fw, kernels=jk + fk)
        else:
            cand, jw, jk, jb = bj.timed(ss, lambda: join(least_seeds))
            t0 = time.perf_counter()
            held = cand.hits(nucleotide_matrix(), 11.0, 2.0, bj.a.f_min)
            hits_ms = (time.perf_counter() - t0) * 1e3
            st = ss.stats()
            t0 = time.perf_counter()
            cg = held.cigars()
            cells_ms = (time.perf_counter() - t0) * 1e3
            out.update(min_seeds=least_seeds, candidates=len(cand), kept=int(np.isin(true_pair, cand.index.astype(np.int64)).sum()), held=len(held),
                       held_true=int(np.isin(true_pair, held.index.astype(np.int64)).sum()), join_wall=jw, join_kernels=jk, join_bytes=jb, hits_wall=hits_ms,
                       hits_fill=st["fill_ms"] + st["refill_ms"], cells_wall=cells_ms, wall=jw + hits_ms + cells_ms)
            # (c): the held hits whose pair the loose list chained, chain extent against aligned region
            pos, there = at_true(loose.index, held.index.astype(np.int64))
            ok = there & (cg.records["status"] == 0)
            ok[ok] = (recs["flags"][pos[ok]] == 0) & (recs["anchors"][pos[ok]] > 0)
            is_true = np.isin(held.index.astype(np.int64), true_pair)
            parts = {}
            for part, sel in (("true overlaps", ok & is_true), ("other pairs", ok & ~is_true)):
                r, c = recs[pos[sel]], cg.records[sel]
                dist = {}
                for name in ("q_start", "q_end", "t_start", "t_end"):
                    d = np.abs(r[name].astype(np.int64) - c[name].astype(np.int64))
                    dist[name] = [float(x) for x in np.percentile(d, [50, 90, 99, 100])] if len(d) else [0.0] * 4
                inside = int(((r["q_start"] >= c["q_start"]) & (r["q_end"] <= c["q_end"]) & (r["t_start"] >= c["t_start"]) & (r["t_end"] <= c["t_end"])).sum())
                parts[part] = dict(compared=int(sel.sum()), distance=dist, chain_inside=inside)
            out.update(parts=parts)
        print(json.dumps(out), flush=True)


def main():
    if a.child:
        child(a.child)
        return 0
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    bj = seedjoin_bench()
    _reads, _q, _t, text = bj.workload()
    say("tools/bench_seedchain.py: seed_join + chain_filter against seed_join + hits + the held hits' cells, k = %d, band %d, max_gap %d, max_skew %d; "
        "a process per route and run, %d alternating runs, median (spread)" % (a.k, bj.a.band, a.max_gap, a.max_skew, a.runs))
    say(text)
    got = {r: [] for r in ROUTES}
    passed = [x for x in sys.argv[1:] if x != "--child"]
    for _ in range(a.runs):
        for r in ROUTES:
            out = subprocess.run([sys.executable, os.path.abspath(__file__)] + passed + ["--child", r], capture_output=True, text=True, timeout=600)
            if out.returncode != 0:                                              # nothing more is started after a failure
                say("%s failed with status %d: %s" % (r, out.returncode, out.stderr[-800:]))
                write(lines)
                return 1
            got[r].append(json.loads(out.stdout.strip().splitlines()[-1]))

    def med(rows, key):
        v = np.array([x[key] for x in rows], dtype=np.float64)
        return "%.2f (%.2f)" % (np.median(v), v.max() - v.min())

    for r in ROUTES:
        rows = got[r]
        x = rows[-1]
        assert all((y["candidates"], y["kept"]) == (x["candidates"], x["kept"]) for y in rows)
        say()
        if r.startswith("chain"):
            say("%s (a): min_score %d, %d candidates (%d at seed threshold 1), %d of %d true overlaps (recall %.4f; %d listed by the join), %d overflowed" % (
                r, x["min_score"], x["candidates"], x["at_threshold_1"], x["kept"], x["true"], x["kept"] / max(x["true"], 1), x["listed_at_1"], x["overflowed"]))
            say("  anchors %(anchors)d, candidates with an anchor %(with_anchor)d, chunks %(chunks)d" % x["chain_summary"])
            say("  join   wall %s ms, kernels %s ms, %d bytes down" % (med(rows, "join_wall"), med(rows, "join_kernels"), x["join_bytes"]))
            say("  filter wall %s ms, kernels %s ms, %d bytes down" % (med(rows, "filter_wall"), med(rows, "filter_kernels"), x["filter_bytes"]))
            say("  both   wall %s ms, kernels %s ms" % (med(rows, "wall"), med(rows, "kernels")))
        else:
            say("%s (b): min_seeds %d, %d candidates, %d of %d true overlaps listed (recall %.4f), %d hits held (%d of the true overlaps)" % (
                r, x["min_seeds"], x["candidates"], x["kept"], x["true"], x["kept"] / max(x["true"], 1), x["held"], x["held_true"]))
            say("  join   wall %s ms, kernels %s ms, %d bytes down" % (med(rows, "join_wall"), med(rows, "join_kernels"), x["join_bytes"]))
            say("  hits   wall %s ms, fills %s ms; start and end cells wall %s ms" % (med(rows, "hits_wall"), med(rows, "hits_fill"), med(rows, "cells_wall")))
            say("  all    wall %s ms" % med(rows, "wall"))
            for part in ("true overlaps", "other pairs"):
                y = x["parts"][part]
                say("  (c) %s, %d held hits whose pair is chained: |chain - aligned| in residues, median / 90 %% / 99 %% / max" % (part, y["compared"]))
                for name in ("q_start", "q_end", "t_start", "t_end"):
                    say("      %-8s %g / %g / %g / %g" % ((name,) + tuple(y["distance"][name])))
                say("      the chain lies inside the aligned region on both records in %d of them" % y["chain_inside"])
    write(lines)
    return 0


def write(lines):
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
