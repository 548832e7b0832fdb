"""No result of a resident pair set may depend on the handle's call history (helpers, catalogue and state model: tests/pairset_history.py).

One handle of 13 protein pairs runs call_history.schedule(18): 325 calls in which every one of the 18 catalogue entries -- five runs
(every pair, a permuted subset under the other semantics, a 4 x 4 run, an empty run, a run cut into chunks), two parameter sets, both
re-estimations, run_stored, five fetches (lists inside and outside run_subset's list, the 4 x 4 run's counts), loop_begin, loop_step
and a pass on the owning sequence set -- directly follows every other one and itself exactly once.  A tail of 1105 calls follows: every
transition the header allows in a state that accepts both calls, and every entry between the first and second and between the second
and third step of a loop.  After every call the whole held run's strings and every written store entry are fetched as well, so that a
corrupted state shows at the call that corrupted it.  Every answer is compared, bit for bit over whole marker-filled arrays, with
values that come from the CPU oracle, tests/transform_ref.py and the restated loop rule; every call the state model refuses must be
refused and must leave its outputs untouched.  The walk runs on a handle that copied its residues and on one that borrows a sequence
set's, each in a child process of its own, and the two logs must be equal call by call; a third child destroys its handle half-way and
goes on with a handle over another pair list on the same context."""
import json
import os
import subprocess
import sys
import time

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import call_history as CH  # noqa: E402
import pairset_history as H  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_SEED, SHORT = 977, 60


@pytest.fixture(scope="module")
def job(orc, tmp_path_factory):
    """the references, once: the plan and the expected arrays of both pair lists, in files the children read"""
    d = tmp_path_factory.mktemp("pairset_history")
    parts = {}
    for tag, seed, calls in (("first", 20261021, None), ("other", OTHER_SEED, SHORT)):
        refs = H.Refs(orc, seed)
        plan = H.dry_run(refs, calls)
        path = str(d / (tag + ".npz"))
        CH.save_expected(path, refs.memo)
        parts[tag] = dict(seed=seed, plan=plan, expected=path)
    assert any(a.tobytes() != b.tobytes() for (a, _x), (b, _y) in zip(H.pair_list(H.records()), H.pair_list(H.records(OTHER_SEED))))
    return d, parts


def run_child(d, mode, parts):
    job_path, report = str(d / (mode + ".json")), str(d / (mode + ".report.json"))
    with open(job_path, "w") as f:
        json.dump(dict(parts=parts), f)
    t0 = time.perf_counter()
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pairset_history.py"), mode, job_path, report], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    with open(report) as f:
        out = json.load(f)
    for w in out["walks"]:
        print("%s: %d calls in %.2f s (%.2f s inside the library's calls; child process %.2f s), refusals %s" % (
            mode, w["calls"], w["seconds"], w["library_seconds"], time.perf_counter() - t0, w["refusals"]))
    return out["walks"]


def describe(w):
    return "\n".join(f["message"] for f in w["failures"][:12]) + "\n(%d failures in %d calls)" % (len(w["failures"]), w["calls"])


@pytest.fixture(scope="module")
def copied(job):
    d, parts = job
    return run_child(d, "copied", [parts["first"]])[0]


@pytest.fixture(scope="module")
def borrowed(job):
    d, parts = job
    return run_child(d, "borrowed", [parts["first"]])[0]


def expected_calls(plan, skip=()):
    return sum(1 + len(x["obs"]) for x in plan if x["entry"] not in skip)


def test_walk_on_copied_residues(job, copied):
    plan = job[1]["first"]["plan"]
    assert not copied["failures"], describe(copied)
    assert copied["calls"] == expected_calls(plan, ("set_pass",)) and all(v >= 1 for v in copied["refusals"].values()), copied["refusals"]


def test_walk_on_borrowed_residues_with_passes_on_the_set(job, borrowed):
    plan = job[1]["first"]["plan"]
    assert not borrowed["failures"], describe(borrowed)
    assert borrowed["calls"] == expected_calls(plan) and all(v >= 1 for v in borrowed["refusals"].values()), borrowed["refusals"]


def test_copied_and_borrowed_answer_the_same_bytes(job, copied, borrowed):
    plan = job[1]["first"]["plan"]
    assert len(copied["log"]) == len(borrowed["log"]) == len(plan)
    differing = [(x["step"], x["prev"], x["entry"]) for x, a, b in zip(plan, copied["log"], borrowed["log"]) if x["entry"] != "set_pass" and a != b]
    assert not differing, differing[:10]
    assert all(a is None and b is not None for x, a, b in zip(plan, copied["log"], borrowed["log"]) if x["entry"] == "set_pass")


def test_destroy_in_the_middle(job):
    """half of the schedule, then the handle is destroyed and a new one over another seeded pair list on the same context runs a short
    schedule: its answers are those of a handle that never saw the first list (the references of the other list alone)"""
    d, parts = job
    half = dict(parts["first"], plan=parts["first"]["plan"][:len(parts["first"]["plan"]) // 2])
    walks = run_child(d, "destroy", [half, parts["other"]])
    assert len(walks) == 2
    for w, plan in zip(walks, (half["plan"], parts["other"]["plan"])):
        assert not w["failures"], describe(w)
        assert w["calls"] == expected_calls(plan, ("set_pass",))
    assert len(parts["other"]["plan"]) == SHORT
