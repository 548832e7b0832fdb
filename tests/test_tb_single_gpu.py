"""The parallel traceback of one large pair (aln_tb_single_{maps,chain,segments,expand}_kernel) on constructed paths: band edges,
clamped bands, border runs, the give-up cap, walks that leave the staged window, start cells on strip edges, tag counts around 1024.

Per case (tests/tb_single_cases.py) the summary and both strings are those of the CPU oracle bit for bit, and the class string of the
`aln tb:` line (ALN_TRACE_TB) is the one tests/tb_single_model.py derives from the oracle's path -- so a strip crossed by another of
the chain kernel's four ways than the geometry demands fails even though the answer is right.  tests/test_tb_single_model_cpu.py
holds every case to the class it is built for.  Pairs of at most 1.5 M cells compare every direction as well.

One child process per route and rows-per-lane setting (ALN_SINGLE_R / ALN_WG_R and ALN_TRACE_TB are read from the environment), all
of its cases on one context; after a child that died or timed out nothing more is started.  The last test runs the single-route
cases of R = 1 three times over on one context -- table order, reversed, largest and smallest N interleaved -- because the exit maps
(`tbmap`) are never cleared between calls: a band bookkeeping that read entries nobody wrote for this pair would take another pair's."""
import hashlib
import json
import os
import re
import subprocess
import sys
import time

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tb_single_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu
HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tb_single_cases.py")
CHILD_TIMEOUT = 240
KNOBS = ("ALN_SINGLE_R", "ALN_WG_R", "ALN_NO_SINGLE", "ALN_NO_WGPIPE", "ALN_BIG_TO_SINGLE", "ALN_NO_COOP", "ALN_SINGLE_W1", "ALN_TRACE_PLAN")
FLAG_SINGLE, FLAG_WORKGROUP = 2, 4
TRACE = re.compile(r"^aln tb: pair (\d+) R (\d+) strips (\d+) classes (\d+)$")
_child_lost = []
_want = {}


def want(orc, case):
    """The oracle's answer and the model's class string of a case, once per session."""
    if case.id not in _want:
        q, t = case.seqs()
        ref = tc.oracle(orc, case, want_matrices=len(q) * len(t) <= tc.DIRECTION_CELLS)
        assert ref["status"] == 0
        strips, classes, moves = tc.run_model(case, ref)
        miss = tc.check_aim(case, strips, classes, moves)
        assert not miss, (case.id, miss)
        _want[case.id] = (ref, classes, hashlib.sha256(ref["D"].tobytes()).hexdigest() if "D" in ref else None)
        ref.pop("H", None), ref.pop("D", None)
    return _want[case.id]


def run_child(what, env_extra, tmp_path):
    assert not _child_lost, "an earlier child process faulted or timed out (%s): nothing more is started" % _child_lost[0]
    report = str(tmp_path / "report.json")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_extra, ALN_TRACE_TB="1")
    t0 = time.perf_counter()
    try:
        p = subprocess.run([sys.executable, HELPER, report, what], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _child_lost.append("no result within %d s" % CHILD_TIMEOUT)
        raise
    if p.returncode != 0:
        _child_lost.append("exit status %d" % p.returncode)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    with open(report) as f:
        got = json.load(f)
    traces, cur = [], None
    for line in p.stderr.splitlines():
        if line.startswith("tb case: "):
            cur = []
            traces.append(cur)
        elif line.startswith("aln tb:"):
            m = TRACE.match(line)
            assert m and cur is not None, line
            cur.append(tuple(int(v) for v in m.groups()[:3]) + (m.group(4),))
    assert len(traces) == len(got)
    print("tb single %s: child %.1f s, %d calls" % (env_extra, time.perf_counter() - t0, len(got)))
    return got, traces


def check(orc, case, g, trace, directions=True):
    ref, classes, d_digest = want(orc, case)
    assert g["id"] == case.id and g["status"] == 0
    assert (g["score"], g["f"]) == (float(ref["score"]).hex(), float(ref["f"]).hex()), (case.id, g["score"], ref["score"])
    assert (tuple(g["end"]), tuple(g["start"])) == (ref["end"], ref["start"]), (case.id, g["end"], g["start"], ref["end"], ref["start"])
    assert g["aln_len"] == len(ref["qa"]), (case.id, g["aln_len"], len(ref["qa"]))
    assert g["qa"] == ref["qa"].tobytes().hex(), (case.id, "query string")
    assert g["ta"] == ref["ta"].tobytes().hex(), (case.id, "target string")
    assert g["flags"] & (FLAG_SINGLE if case.route == "single" else FLAG_WORKGROUP), (case.id, g["flags"])
    ns = (len(case.seqs()[1]) + 64 * case.R - 1) // (64 * case.R)
    print("%-36s classes %s" % (case.id, trace[-1][3] if trace else None))
    # (the last line: a process's first call also shows the pair the context warms up with)
    assert trace[-1:] == [(0, case.R, ns, classes)], (case.id, trace, classes)
    if directions and d_digest is not None:
        assert g["D"] == d_digest, (case.id, "directions")


GROUPS = [("single", 1, {"ALN_SINGLE_R": "1"}), ("single", 2, {"ALN_SINGLE_R": "2"}),
          ("wg", 1, {"ALN_WG_R": "1"}), ("wg", 2, {"ALN_WG_R": "2"}), ("wg", 4, {"ALN_WG_R": "4"})]


@pytest.mark.parametrize("route,R,env", GROUPS, ids=["%s_R%d" % g[:2] for g in GROUPS])
def test_constructed_paths_against_oracle_and_model(orc, tmp_path, route, R, env):
    cases = [c for c in tc.cases() if c.route == route and c.R == R]
    assert cases
    for c in cases:
        want(orc, c)
    got, traces = run_child(",".join(c.id for c in cases) + "+d", env, tmp_path)
    for c, g, tr in zip(cases, got, traces):
        check(orc, c, g, tr)


def test_pwm_window_on_the_one_workgroup_route(orc, tmp_path):
    """As test_pwm_aligner_matches_oracle: no seed pair, `numbered` in place of the query string."""
    seq, pwm = tc.pwm_case()
    ref = orc.align_pwm(seq, tc.PWM_DEL, tc.PWM_EXT, pwm)
    _, classes, _ = tc.pwm_model(ref)
    got, traces = run_child("pwm", {"ALN_WG_R": str(tc.PWM_R)}, tmp_path)
    g = got[0]
    assert g["status"] == 0 and (g["score"], g["f"]) == (float(ref["score"]).hex(), float(ref["f"]).hex())
    assert (tuple(g["end"]), tuple(g["start"])) == (ref["end"], ref["start"]) and g["aln_len"] == len(ref["numbered"])
    assert g["qa"] == ref["numbered"].astype("<u4").tobytes().hex() and g["ta"] == ref["qal"].tobytes().hex()
    assert g["flags"] & FLAG_WORKGROUP
    assert traces[0][-1:] == [(0, tc.PWM_R, (1500 + 64 * tc.PWM_R - 1) // (64 * tc.PWM_R), classes)], (traces[0], classes)


def test_results_do_not_depend_on_the_pairs_traced_before(orc, tmp_path):
    cases = [c for c in tc.cases() if c.route == "single" and c.R == 1]
    by_n = sorted(cases, key=lambda c: len(c.seqs()[0]))
    mixed = [c for pair in zip(reversed(by_n), by_n) for c in pair][:len(cases)]
    order = cases + cases[::-1] + mixed
    assert {c.id for c in mixed} == {c.id for c in cases}
    got, traces = run_child(",".join(c.id for c in order), {"ALN_SINGLE_R": "1"}, tmp_path)
    for c, g, tr in zip(order, got, traces):
        check(orc, c, g, tr, directions=False)
