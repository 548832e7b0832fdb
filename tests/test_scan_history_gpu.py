"""No result of a window scan may depend on the scan's call history (helpers, catalogue and state model: tests/scan_history.py).

One scan over a seeded chromosome of 3001 codes runs call_history.schedule(23): 530 calls in which every one of the 23 catalogue
entries -- two score passes, four select passes (one over capacity), eight held passes (forward and reverse, integer and real-valued
PWMs, every window a hit, none, two-strip windows, four windows on the one-workgroup route on both strands, no window at all), two
refused passes, six fetches and a held pass with its fetches on a second scan over another chromosome of the same length -- directly
follows every other one and itself exactly once.  After every call the whole held list and every hit's strings are fetched as well
(or, where nothing may be held, an empty range, which must be refused), so that a corrupted state shows at the call that corrupted
it.  Every answer is compared, bit for bit over whole marker-filled arrays, with the CPU oracle window by window; every call the
state model refuses must be refused and must leave its outputs untouched.  The catalogue uses 13 plan keys, so the process-wide cache
of 8 plans evicts and plans again throughout.  A second child destroys its scan half-way and goes on with a scan over the other
chromosome on the same context; a third runs 1100 passes (1650 launches) on one scan's slot, so that its salt wraps.

Every child runs in a process of its own, one at a time and under its own time limit; when a child dies or times out its test fails
and the tests after it fail without starting anything."""
import json
import os
import re
import subprocess
import sys
import time

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import call_history as CH  # noqa: E402
import scan_history as H  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 120
SHORT = 60
ROUTE = re.compile(r"aln route: pairs (\d+) small (\d+) single (\d+) wg (\d+) .* kernels (\w+)")
MARKER = re.compile(r"scan call (\d+) (\w+)")
_child_lost = []


@pytest.fixture(scope="module")
def job(orc, tmp_path_factory):
    """the references, once: the plan and the expected arrays of both chromosomes, in files the children read"""
    d = tmp_path_factory.mktemp("scan_history")
    parts = {}
    for tag, seed, other, calls in (("first", H.SEED, H.OTHER_SEED, None), ("other", H.OTHER_SEED, H.SEED, SHORT)):
        refs = H.Refs(orc, seed, other)
        plan = H.dry_run(refs, calls)
        path = str(d / (tag + ".npz"))
        CH.save_expected(path, refs.memo)
        parts[tag] = dict(seed=seed, other_seed=other, length=H.LEN, plan=plan, expected=path)
    return d, parts


def run_child(d, mode, job):
    assert not _child_lost, "an earlier child process faulted or timed out (%s): nothing more is started" % _child_lost[0]
    job_path, report = str(d / (mode + ".json")), str(d / (mode + ".report.json"))
    with open(job_path, "w") as f:
        json.dump(job, f)
    env = dict(os.environ, ALN_TRACE_PLAN="1")
    t0 = time.perf_counter()
    try:
        run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scan_history.py"), mode, job_path, report], env=env, capture_output=True,
                             text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _child_lost.append("%s: no result within %d s" % (mode, CHILD_TIMEOUT))
        raise
    if run.returncode != 0:
        _child_lost.append("%s: exit status %d" % (mode, run.returncode))
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    with open(report) as f:
        out = json.load(f)
    for w in out.get("walks", []):
        print("%s: %d calls in %.2f s (%.2f s inside the library's calls; child process %.2f s), refusals %s" % (
            mode, w["calls"], w["seconds"], w["library_seconds"], time.perf_counter() - t0, w["refusals"]))
    return out, run.stderr


def describe(w):
    return "\n".join(f["message"] for f in w["failures"][:12]) + "\n(%d failures in %d calls)" % (len(w["failures"]), w["calls"])


def routes_per_call(stderr):
    """[(entry, [(pairs, small, single, wg, kernels)])] per call of the child, from its own marker lines and the library's route lines"""
    calls = []
    for line in stderr.splitlines():
        m = MARKER.match(line)
        if m:
            calls.append((m.group(2), []))
            continue
        r = ROUTE.match(line)
        if r and calls:
            calls[-1][1].append((int(r.group(1)), int(r.group(2)), int(r.group(3)), int(r.group(4)), r.group(5)))
    return calls


def test_walk(job):
    d, parts = job
    part = parts["first"]
    out, stderr = run_child(d, "walk", dict(parts=[part]))
    w, plan = out["walks"][0], part["plan"]
    assert not w["failures"], describe(w)
    assert w["calls"] == H.expected_calls(plan) and all(v >= 1 for v in w["refusals"].values()), w["refusals"]
    k = len(H.CATALOGUE)
    assert len(plan) == k * k + 1 and CH.transitions(w["entries"]) == {(a, b) for a in H.CATALOGUE for b in H.CATALOGUE}
    calls = routes_per_call(stderr)
    assert len(calls) == w["calls"]
    lines = [r for _e, rs in calls for r in rs]
    assert any(r[4] == "fast" for r in lines) and any(r[4] == "f64" for r in lines) and any(r[3] > 0 for r in lines), lines[:20]
    # a pass that had run before was planned again (its plan had been evicted), and some pass was not planned at all (a cache hit)
    seen, replanned, cached = set(), 0, 0
    for entry, rs in calls:
        if entry not in H.PASSES or entry == "hits_no_window":
            continue
        if rs and entry in seen:
            replanned += 1
        if not rs:
            cached += 1
        seen.add(entry)
    print("walk: %d route lines, %d passes planned again after an eviction, %d passes served from the cache" % (len(lines), replanned, cached))
    assert replanned >= 1 and cached >= 1


def test_destroy_in_the_middle(job):
    """half of the schedule, then the scan is destroyed and a new one over the other chromosome on the same context runs a short schedule:
    its answers are those of a scan that never saw the first chromosome (the references of its own alone)"""
    d, parts = job
    half = dict(parts["first"], plan=parts["first"]["plan"][:len(parts["first"]["plan"]) // 2])
    out, _stderr = run_child(d, "destroy", dict(parts=[half, parts["other"]]))
    walks = out["walks"]
    assert len(walks) == 2
    for w, plan in zip(walks, (half["plan"], parts["other"]["plan"])):
        assert not w["failures"], describe(w)
        assert w["calls"] == H.expected_calls(plan)
    assert len(parts["other"]["plan"]) == SHORT


def test_more_than_1024_launches_on_one_scan(orc, job):
    d, _parts = job
    args, wants = H.wrap_args(orc)
    path = str(d / "wrap.npz")
    CH.save_expected(path, wants)
    t0 = time.perf_counter()
    r, _stderr = run_child(d, "wrap", dict(seed=H.SEED, passes=H.WRAP_PASSES, args=args, expected=path))
    print("wrap: %s (child process %.2f s)" % ({k: v for k, v in r.items() if k != "first_bad"}, time.perf_counter() - t0))
    assert r["bad"] == 0, "%d passes differ from the oracle; (pass, PWM, what): %s" % (r["bad"], r["first_bad"])
    assert r["passes"] >= 1100 and r["launches"] > 1024 + 50
