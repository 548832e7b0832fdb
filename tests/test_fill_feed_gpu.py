"""The fast batch kernel's per-step feed at the boundaries of its LDS query ring and of its 64-column input chunks.
Every lane reads its column's query code from a 256-entry ring that is refilled 64 columns at a time (aln_fast.h), and a strip
below strip 0 takes the row above it 64 columns at a time.  Pairs whose query has 1, 63, 64, 65, 127, 128, 129, 255, 256, 257
and 2047 .. 2049 columns (chunk ends, ring wrap, the end-cell tracker's 2048-step chunk) against targets of 1, 511, 512, 513
and 1025 rows (one lane, one strip short of full, exactly full, a strip above a one-row strip, two strips above), core local
(11 / 2: the row-1 hazard machinery runs too) and core global, on the lean and on the cooperative build of the kernel: summary
and both aligned strings of every pair against the oracle.  ALN_COOP_LEAN is read once per process, so each build runs in a
child process of its own, one at a time and under its own time limit; when a child dies or times out the test fails and the
cases after it fail without starting anything."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from aligner_amd import _ffi
from aligner_amd.batch import PairBatch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049)
ROWS = (1, 511, 512, 513, 1025)
SEMANTICS = (("core_local", _ffi.CORE_LOCAL), ("core_global", _ffi.CORE_GLOBAL))
DEL, EXT = 11, 2
CHILD_TIMEOUT = 300
PLAN = re.compile(r"aln plan: .* build (\w+)")
_child_lost = []

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[2])
from aligner_amd.batch import PairBatch, align_batch
from aligner_amd.matrices import get_blosum62
b = PairBatch(*[np.load(sys.argv[3])[k] for k in ("seqs", "q_off", "q_len", "t_off", "t_len")])
out = {}
for sem in sys.argv[4:]:
    r = align_batch(b, int(sem), 11, 2, get_blosum62())
    out["results" + sem] = r.results
    out["strings" + sem] = np.concatenate([np.concatenate(r.aligned(i)) for i in range(len(b))])
np.savez(sys.argv[1], **out)
"""


def related(rng, n, m, A=20):
    """A query of n letters and a target of m letters made of runs copied from it, with some letters changed and random letters
    between the runs: alignments that cross chunk and strip boundaries."""
    q = rng.integers(0, A, n).astype(np.uint8)
    t = []
    while len(t) < m:
        L = int(rng.integers(20, 120))
        s = int(rng.integers(0, max(1, n - L)))
        run = q[s:s + L].copy()
        mut = rng.random(len(run)) < 0.05
        run[mut] = rng.integers(0, A, int(mut.sum()))
        t.extend(run.tolist())
        t.extend(rng.integers(0, A, int(rng.integers(0, 6))).tolist())
    return q, np.array(t[:m], dtype=np.uint8)


def shapes():
    return [(n, m) for n in COLS for m in ROWS]


def boundary_batch():
    rng = np.random.default_rng(20260517)
    return PairBatch.from_pairs([related(rng, n, m) for n, m in shapes()])


@pytest.mark.parametrize("lean", [1, 0], ids=["lean", "cooperative"])
def test_ring_and_chunk_boundaries_against_the_oracle(orc, blosum62, tmp_path, lean):
    assert not _child_lost, "an earlier child process faulted or timed out (%s): nothing more is started" % _child_lost[0]
    b = boundary_batch()
    assert len(b) == len(COLS) * len(ROWS)
    np.savez(tmp_path / "batch.npz", seqs=b.seqs, q_off=b.q_off, q_len=b.q_len, t_off=b.t_off, t_len=b.t_len)
    out = tmp_path / "out.npz"
    env = dict(os.environ, ALN_COOP_LEAN=str(lean), ALN_TRACE_PLAN="1")
    cmd = [sys.executable, "-c", CHILD, str(out), ROOT, str(tmp_path / "batch.npz")] + [str(sem) for _, sem in SEMANTICS]
    try:
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _child_lost.append("build lean=%d: no result within %d s" % (lean, CHILD_TIMEOUT))
        raise
    if p.returncode != 0:
        _child_lost.append("build lean=%d: exit status %d" % (lean, p.returncode))
    assert p.returncode == 0, p.stdout + p.stderr
    builds = PLAN.findall(p.stderr)
    assert builds and set(builds) == {"lean" if lean else "coop"}, p.stderr
    got = np.load(out)
    for name, sem in SEMANTICS:
        res, strings = got["results%d" % sem], got["strings%d" % sem]
        offs = np.concatenate([[0], np.cumsum(2 * res["aln_len"].astype(np.int64))])
        ref, tb, tb_off = orc.align_batch(sem, b.seqs, b.q_off, b.q_len, b.t_off, b.t_len, DEL, EXT, blosum62, n_threads=8)
        for i, (n, m) in enumerate(shapes()):
            case = (name, "N=%d" % n, "M=%d" % m)
            r, g = ref[i], res[i]
            assert g["status"] == r.status == 0, case
            # the fast batch kernel, not the single-pair route
            assert g["flags"] & _ffi.FLAG_FAST and not g["flags"] & _ffi.FLAG_SINGLE, (case, int(g["flags"]))
            assert (g["score"], g["f"], g["end_y"], g["end_x"], g["start_y"], g["start_x"], g["aln_len"]) == \
                   (r.score, r.f, r.end_y, r.end_x, r.start_y, r.start_x, r.aln_len), case
            s = strings[offs[i]:offs[i + 1]]
            qa, ta = s[:len(s) // 2], s[len(s) // 2:]
            cap = n + m + 2
            o = int(tb_off[i])
            assert (qa == tb[o:o + r.aln_len]).all() and (ta == tb[o + cap:o + cap + r.aln_len]).all(), case
