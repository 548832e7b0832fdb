"""The two builds of the fast batch kernel compute the same thing, and the library picks the lean one for C5.
* 3 000 C5 pairs run with the lean build forced (ALN_COOP_LEAN=1, no cooperative machinery) equal the same batch with the
  cooperative build forced (ALN_COOP_LEAN=0) -- every summary field and the aligned strings of every pair.  Under two pairs per
  resident wave, so the cooperative run shares first passes and re-fills.  The plan's trace (ALN_TRACE_PLAN) shows that the two
  runs did take different builds.
* The full C5 batch, staged as bench.py stages it, is planned onto the lean build with the figures of aln_coop_lean_plan: 3072
  kernel waves (the walk runs beside the fill: the grid is the resident workgroups) and the tail from queue position 100000 - 6144.
The settings are read once per process: each run is a fresh child process."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[2])
from aligner_amd import _ffi, workloads
from aligner_amd.batch import align_batch
from aligner_amd.matrices import get_blosum62
b = workloads.c5_batch(3000)
r = align_batch(b, _ffi.CORE_LOCAL, 11, 2, get_blosum62())
strings = np.concatenate([np.concatenate(r.aligned(i)) for i in range(len(b))])
np.savez(sys.argv[1], results=r.results, strings=strings)
"""

CHILD_C5 = r"""
import sys
sys.path.insert(0, sys.argv[1])
from aligner_amd import _ffi, workloads
from aligner_amd.batch import StagedBatch
from aligner_amd.matrices import get_blosum62
sb = StagedBatch(workloads.c5_batch(100000), _ffi.CORE_LOCAL, 11, 2, get_blosum62(), outputs=3)
sb.run(); sb.sync()
r = sb.fetch(False).results
assert (r["status"] == 0).all()
"""

PLAN = re.compile(r"aln plan: pairs (\d+) waves (\d+) resident (\d+) tail (\d+) share \S+ tail_cost \d+ max_cost \d+ build (\w+)")


def plans(stderr):
    return [m.groups() for m in PLAN.finditer(stderr)]


def run_child(tmp_path, lean):
    out = str(tmp_path / ("lean%d.npz" % lean))
    env = dict(os.environ, ALN_COOP_LEAN=str(lean), ALN_TRACE_PLAN="1")
    p = subprocess.run([sys.executable, "-c", CHILD, out, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    return np.load(out), plans(p.stderr)


@pytest.mark.gpu
def test_lean_build_equals_cooperative_build(tmp_path):
    (coop, coop_plans), (lean, lean_plans) = run_child(tmp_path, 0), run_child(tmp_path, 1)
    assert coop_plans and all(pl[-1] == "coop" for pl in coop_plans), coop_plans
    assert lean_plans and all(pl[-1] == "lean" for pl in lean_plans), lean_plans
    rc, rl = coop["results"], lean["results"]
    assert (rc["status"] == 0).all()
    for f in ("status", "score", "f", "end_y", "end_x", "start_y", "start_x", "aln_len"):
        assert np.array_equal(rc[f], rl[f]), f
    assert np.array_equal(coop["strings"], lean["strings"])


@pytest.mark.gpu
def test_c5_is_planned_onto_the_lean_build():
    env = dict(os.environ, ALN_TRACE_PLAN="1")
    env.pop("ALN_COOP_LEAN", None)
    p = subprocess.run([sys.executable, "-c", CHILD_C5, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    pl = plans(p.stderr)
    assert len(pl) == 1, p.stderr
    pairs, waves, resident, tail, build = pl[0]
    assert (int(pairs), int(waves), int(resident), int(tail), build) == (100000, 3072, 3072, 100000 - 2 * 3072, "lean")
