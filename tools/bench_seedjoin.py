"""The seed join against the word join as a candidate rule for read overlaps, on both strands.

Workload: a random genome (--genome bases) into which --families repeat families are planted (--copies copies of a --repeat-len element
each, every copy with --repeat-div substitutions); --reads reads of --read-len bases sampled at uniform positions, on a random strand,
each with --sub-rate substitutions and --indel-rate single-base indels.  A true overlap is an ordered pair of different reads whose
genome intervals share --min-overlap bases or more; on the stranded set (n reads, 2n resident records) it is the pair (i, j) if both
reads come from one strand and (i, n + j) if not.  The block is every read against all 2n records.

Routes: word_index + word_join at k = 8 (min_shared), and seed_index + seed_join at k = 8 and k = 12 .. 15 (min_seeds, --band), and at
k = 12 and 15 once more with --max-occ (seed12o, seed15o).  Every
threshold is the largest value that still lists every true overlap the route lists at threshold 1: the least count over the true
overlaps, found by a first call at threshold 1 in the same process (it also warms the kernels).  Then, timed: the index, the join at
that threshold, and the `hits` pass over the list (nucleotide matrix, --f-min).  Per route: candidates kept, recall of the true
overlaps, kernel and wall time of index and join, bytes down, the time of hits and the hits held.

Every (route, run) is a process of its own (--child); the routes alternate, --runs times; the medians and spreads go to --out.
usage: python tools/bench_seedjoin.py [--reads 2000] [--runs 3] [--out profiles/r23_seedjoin.txt]"""
import argparse, json, os, subprocess, sys, time
sys.path.insert(0, ".")
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--genome", type=int, default=200000)
ap.add_argument("--families", type=int, default=4)
ap.add_argument("--copies", type=int, default=40)
ap.add_argument("--repeat-len", type=int, default=300)
ap.add_argument("--repeat-div", type=float, default=0.05)
ap.add_argument("--reads", type=int, default=2000)
ap.add_argument("--read-len", default="300,600")
ap.add_argument("--sub-rate", type=float, default=0.02)
ap.add_argument("--indel-rate", type=float, default=0.005)
ap.add_argument("--min-overlap", type=int, default=100)
ap.add_argument("--band", type=int, default=8)
ap.add_argument("--max-occ", type=int, default=40, help="of the routes whose name ends in o: words with more occurrences in the set make no seed")
ap.add_argument("--f-min", type=float, default=200.0)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--seed", type=int, default=23)
ap.add_argument("--out", default="profiles/r23_seedjoin.txt")
ap.add_argument("--child", default=None, help="one route in this process: word8, seed8, seed12, ...; prints one JSON line")
a = ap.parse_args()
ROUTES = ["word8", "seed8", "seed12", "seed13", "seed14", "seed15", "seed12o", "seed15o"]          # ...o: with --max-occ


def workload():
    """(reads as code arrays, ordered true overlaps as (q, resident t) arrays, a description)"""
    from aligner_amd.enums import DNA
    comp = DNA.complement_map()
    rng = np.random.default_rng(a.seed)
    genome = rng.integers(0, 4, a.genome).astype(np.uint8)
    covered = 0
    for _ in range(a.families):
        element = rng.integers(0, 4, a.repeat_len).astype(np.uint8)
        for at in rng.integers(0, a.genome - a.repeat_len, a.copies):
            copy = element.copy()
            flip = rng.random(a.repeat_len) < a.repeat_div
            copy[flip] = rng.integers(0, 4, int(flip.sum()))
            if rng.random() < 0.5:
                copy = comp[copy[::-1]]                                          # a copy on the other strand
            genome[at:at + a.repeat_len] = copy
            covered += a.repeat_len
    lo, hi = [int(x) for x in a.read_len.split(",")]
    n = a.reads
    length = rng.integers(lo, hi + 1, n)
    start = rng.integers(0, a.genome - hi, n)
    minus = rng.random(n) < 0.5
    reads = []
    for i in range(n):
        s = genome[start[i]:start[i] + length[i]].copy()
        if minus[i]:
            s = comp[s[::-1]]
        sub = rng.random(len(s)) < a.sub_rate
        s[sub] = rng.integers(0, 4, int(sub.sum()))
        keep = rng.random(len(s)) >= a.indel_rate / 2                            # deletions
        s = s[keep]
        ins = np.flatnonzero(rng.random(len(s)) < a.indel_rate / 2)              # insertions
        s = np.insert(s, ins, rng.integers(0, 4, len(ins)).astype(np.uint8))
        reads.append(s.astype(np.uint8))
    order = np.argsort(start, kind="stable")
    q, t = [], []
    for x, i in enumerate(order):
        for j in order[x + 1:]:
            if start[j] >= start[i] + length[i]:
                break
            if min(start[i] + length[i], start[j] + length[j]) - start[j] >= a.min_overlap:
                for u, v in ((i, j), (j, i)):
                    q.append(u)
                    t.append(v if minus[u] == minus[v] else n + v)
    text = ("%d reads of %s bases (%d residues) from a genome of %d with %d repeat families of %d copies of %d bases (%.1f %% of it), both strands; "
            "%d ordered true overlaps of %d bases or more among %d pairs" % (n, a.read_len, sum(len(r) for r in reads), a.genome, a.families, a.copies,
                                                                             a.repeat_len, 100.0 * covered / a.genome, len(q), a.min_overlap, n * 2 * n))
    return reads, np.array(q, dtype=np.int64), np.array(t, dtype=np.int64), text


def timed(ss, call):
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    st = ss.stats()
    return out, wall, st["fetch_kernel_ms"], st["bytes_down"]


def child(route):
    from aligner_amd.enums import DNA
    from aligner_amd.matrices import nucleotide_matrix
    from aligner_amd.seqset import SeqSet, both, rectangle
    reads, tq, tt, _text = workload()
    n = len(reads)
    true_pair = np.sort(tq * (2 * n) + tt)                                       # pair numbers of the rectangle
    k = int(route[4:].rstrip("o"))
    max_occ = a.max_occ if route.endswith("o") else 0
    with SeqSet.stranded(reads, DNA) as ss:
        block = both(rectangle(0, n, 0, n), n)
        if route.startswith("word"):
            index = lambda: ss.word_index(k, 4)
            join = lambda least: ss.word_join(k, 4, min_shared=least, block=block)
        else:
            index = lambda: ss.seed_index(k, 4)
            join = lambda least: ss.seed_join(k, 4, min_seeds=least, band=a.band, max_occ=max_occ, block=block)
        index()
        loose = join(1)                                                          # threshold 1: what the route can list at all, and the warm call
        at = np.searchsorted(loose.index, true_pair)
        at[at >= len(loose)] = 0
        listed = loose.index[at].astype(np.int64) == true_pair if len(loose) else np.zeros(len(true_pair), dtype=bool)
        least = int(loose.shared[at[listed]].min()) if listed.any() else 1
        loose_count = len(loose)
        del loose
        _, iw, ik, ib = timed(ss, index)
        cand, jw, jk, jb = timed(ss, lambda: join(least))
        kept = int(np.isin(true_pair, cand.index.astype(np.int64)).sum())
        summary = cand.summary
        t0 = time.perf_counter()
        held = cand.hits(nucleotide_matrix(), 11.0, 2.0, a.f_min)
        hits_ms = (time.perf_counter() - t0) * 1e3
        st = ss.stats()
        print(json.dumps(dict(route=route, threshold=least, at_threshold_1=loose_count, listed_at_1=int(listed.sum()), candidates=len(cand), true=len(true_pair),
                              kept=kept, index_wall=iw, index_kernels=ik, index_bytes=ib, join_wall=jw, join_kernels=jk, join_bytes=jb, summary=summary,
                              hits_wall=hits_ms, hits_fill=st["fill_ms"] + st["refill_ms"], held=len(held))), flush=True)


def main():
    if a.child:
        child(a.child)
        return
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    _reads, _q, _t, text = workload()
    say("tools/bench_seedjoin.py: seed_index + seed_join (band %d) against word_index + word_join; a process per route and run, %d alternating runs, median (spread)" % (a.band, a.runs))
    say(text)
    say("thresholds: the least count over the true overlaps the route lists at threshold 1; hits: nucleotide matrix, del 11 / ext 2, f >= %g" % a.f_min)
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
        assert all((y["threshold"], y["candidates"], y["kept"], y["held"]) == (x["threshold"], x["candidates"], x["kept"], x["held"]) for y in rows)
        say()
        say("%s: threshold %d, %d candidates (%d at threshold 1), %d of %d true overlaps (recall %.4f; %d listed at threshold 1), %d hits held" % (
            r, x["threshold"], x["candidates"], x["at_threshold_1"], x["kept"], x["true"], x["kept"] / max(x["true"], 1), x["listed_at_1"], x["held"]))
        if x["summary"]:
            say("  seeds %(seeds)d, pairs with a seed %(pairs_with_seed)d, words dropped %(words_dropped)d, chunks %(chunks)d" % x["summary"])
        say("  index  wall %s ms, kernels %s ms, %d bytes down" % (med(rows, "index_wall"), med(rows, "index_kernels"), x["index_bytes"]))
        say("  join   wall %s ms, kernels %s ms, %d bytes down" % (med(rows, "join_wall"), med(rows, "join_kernels"), x["join_bytes"]))
        say("  hits   wall %s ms, fills %s ms" % (med(rows, "hits_wall"), med(rows, "hits_fill")))
    write(lines)
    return 0


def write(lines):
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
