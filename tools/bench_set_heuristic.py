"""Heuristic alignment of every pair i < j of S proteins (lengths as the C5 workload's, related by planted stretches), BLOSUM62,
del = ext: (a) heuristic.align_many(pairs, transform="resident") on the explicit pair list, which packs both sequences per pair,
against (b) heuristic.align_set on the resident sequence set, which borrows the set's residues and takes the loop's decision on the
device.  Three alternating runs each; per form wall time, iterations, bytes up and down, and the residues held on the device.
usage: python tools/bench_set_heuristic.py [S=300] [--set-only] [--max-pairs N]"""
import sys, time
sys.path.insert(0, ".")
import numpy as np
from aligner_amd import heuristic, workloads
from aligner_amd.enums import Protein
from aligner_amd.matrices import get_blosum62
from aligner_amd.pairset import PairSet
from aligner_amd.seqset import SeqSet
from aligner_amd.simple import Heuristics

args = [a for a in sys.argv[1:] if not a.startswith("--")]
S = int(args[0]) if args else 300
set_only = "--set-only" in sys.argv
max_pairs = int(sys.argv[sys.argv.index("--max-pairs") + 1]) if "--max-pairs" in sys.argv else 1 << 18
DEL = EXT = 8.0
rng = np.random.default_rng(2026)
lens = workloads.c5_lengths(S)[0][:S]
seqs = [rng.integers(0, 20, int(n)).astype(np.uint8) for n in lens]
for i in range(1, S):                                                # a mutated stretch of the sequence before: alignments worth iterating on
    L = int(min(len(seqs[i]), len(seqs[i - 1]), 150))
    piece = seqs[i - 1][:L].copy()
    mut = rng.random(L) < 0.3
    piece[mut] = rng.integers(0, 20, int(mut.sum()))
    seqs[i][-L:] = piece
every = np.concatenate(seqs)
h = Heuristics(-0.5, 576.0, np.bincount(every, minlength=24).astype(np.float64) / len(every))
M = get_blosum62()
n_pairs = S * (S - 1) // 2
print("S = %d, %d pairs, %d residues in the set, %d over the pairs" % (S, n_pairs, len(every), (S - 1) * len(every)))

acc = {}


def tally(ps, name):
    st = ps.stats()
    acc["up"] = acc.get("up", 0) + st["bytes_up"]
    acc["down"] = acc.get("down", 0) + st["bytes_down"]
    if name in ("run_stored", "loop_step"):
        acc["iterations"] = acc.get("iterations", 0) + 1


NAMES = ("set_heuristics", "reestimate", "run_stored", "matrices", "strings", "loop_begin", "loop_step")


class Counted:
    """A pair set whose calls are tallied: delegates everything to the PairSet it wraps."""

    def __init__(self, ps):
        self.ps = ps
        tally(ps, "create")

    def __getattr__(self, name):
        inner = getattr(self.ps, name)
        if name not in NAMES:
            return inner

        def call(*a, **kw):
            r = inner(*a, **kw)
            tally(self.ps, name)
            return r
        return call


def from_pairs(pairs, device=None):
    ps = PairSet(pairs, device)
    acc["residues"] = acc.get("residues", 0) + ps.stats()["bytes_up"]          # packed per pair, uploaded by the create
    return Counted(ps)


def from_set(ss, b, first, n):
    acc["slices"] = acc.get("slices", 0) + 1
    return Counted(PairSet.from_seqset(ss, b, first, n))                      # borrows: the residues are the set's


def explicit():
    pairs = [(seqs[i], seqs[j]) for i in range(S) for j in range(i + 1, S)]
    return heuristic.align_many(pairs, DEL, EXT, M, h, Protein, transform="resident", errors="return", backend=from_pairs)


def on_set():
    with SeqSet(seqs) as ss:
        acc["residues"] = int(ss.len.sum())                                    # every sequence once, uploaded by the set's create
        acc["up"] = acc.get("up", 0) + ss.stats()["bytes_up"]
        return [r for _, _, _, r in heuristic.align_set(ss, DEL, EXT, M, h, max_pairs=max_pairs, backend=from_set)]


got = {}
for rep in range(3):
    for name, fn in (("explicit", explicit), ("set", on_set)):
        if name == "explicit" and set_only:
            continue
        acc.clear()
        t0 = time.perf_counter()
        got[name] = fn()
        wall = time.perf_counter() - t0
        print("run %d %-8s: %9.1f ms wall, %3d iterations, %12d bytes up, %12d bytes down, %12d residue bytes held on the device%s"
              % (rep, name, wall * 1e3, acc.get("iterations", 0), acc.get("up", 0), acc.get("down", 0), acc.get("residues", 0),
                 ", %d slices (iterations are summed over the slices: comparable with the explicit form for one slice only)" % acc["slices"]
                 if "slices" in acc else ""))
if set_only:
    print("the explicit form was not run")
else:
    same = all((isinstance(a, Exception) and isinstance(b, Exception)) or
               (a.alignment.f == b.alignment.f and a.matrix.tobytes() == b.matrix.tobytes() and a.alignment.query.tobytes() == b.alignment.query.tobytes())
               for a, b in zip(got["explicit"], got["set"]))
    print("both forms give the same results: %s" % same)
