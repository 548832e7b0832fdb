"""Residue-code validation on every fill route, at the edges of every site's scan: the catalogue of tests/code_validation_cases.py
through the C ABI (aln_align_batch, aln_align_pair, aln_pairset_run, the PWM batch call), compared with the CPU oracle bit for bit.

Per route one test: every batch's `aln route:` line (ALN_TRACE_PLAN) must be the planned one and must show the route's kernels, every
line's pair must be on the route's list, the flags word of every pair that succeeded must name those kernels, every bad line must come
back ALN_ERR_CODE_OUT_OF_RANGE with the summary of skip_invalid and its string region untouched, and every twin, every legal non-square
line and every neighbour must equal the oracle in every summary field and both strings.  A batch that ran elsewhere fails.

The knobs are read once per process, so the routes run in child processes started fresh, one per environment (the lean build has its
own); a child runs under its own timeout, the parent checks its exit status, and after a child that died or timed out nothing more
is started."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import code_validation_cases as cv  # noqa: E402
import route_cases as rc  # noqa: E402
from test_set_routes_gpu import KNOBS  # noqa: E402

pytestmark = pytest.mark.gpu
HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "code_validation_cases.py")
CHILD_TIMEOUT = 240
ROUTES = [r.name for r in cv.routes()]
_child_lost = []
_children = {}


def child_of(rt, tmp_path_factory):
    """The answers of every route that shares rt's environment, from one child process: ({batch|key: array}, {batch: route lines})"""
    key = tuple(sorted(rt.env.items()))
    if key in _children:
        return _children[key]
    assert not _child_lost, "an earlier child process faulted or timed out (%s): nothing more is started" % _child_lost[0]
    names = [r.name for r in cv.routes() if r.env == rt.env]
    report = str(tmp_path_factory.mktemp("code_validation") / "report.npz")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS + ("ALN_BIG_TO_SINGLE", "ALN_TB_OVERLAP_ANY", "ALN_TRACE_PLAN")}
    env.update(rt.env)
    t0 = time.perf_counter()
    try:
        p = subprocess.run([sys.executable, HELPER, report] + names, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _child_lost.append("%s: no result within %d s" % (names, CHILD_TIMEOUT))
        raise
    if p.returncode != 0:
        _child_lost.append("%s: exit status %d" % (names, p.returncode))
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    with np.load(report) as z:
        got = {k: z[k] for k in z.files}
    print("code validation, %s: child %.1f s" % (names, time.perf_counter() - t0))
    _children[key] = (got, rc.cut_by_call(p.stderr))
    return _children[key]


@pytest.mark.parametrize("name", ROUTES)
def test_every_line_of_the_route(orc, tmp_path_factory, name):
    rt = cv.route(name)
    answers, route_lines = child_of(rt, tmp_path_factory)
    problems, seen = [], 0
    for b in cv.batches(rt):
        got = {k: answers["%s|%s" % (b.name, k)] for k in ("results", "tb", "call")}
        assert int(got["call"]) == 0, (b.name, int(got["call"]))
        lines = route_lines[b.name]
        assert len(lines) == 1, (b.name, lines)
        if seen < 3:
            print("%-28s %s" % (b.name, " ".join("%s %s" % kv for kv in lines[0].items())))
        seen += 1
        problems += cv.route_problems(b, lines[0])
        problems += cv.flag_problems(b, got)
        problems += ["%s: %s" % p for p in cv.check(b, got, cv.expected(orc, b))]
        refused = [ln.name for i, ln in b.lines.items() if ln.bad and got["results"]["status"][i] != cv.REFUSED]
        problems += ["%s: not refused" % n for n in refused]
    assert not problems, "%d problems, first: %s" % (len(problems), problems[:6])
