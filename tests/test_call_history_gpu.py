"""No result may depend on what a slot ran before, nor on a wrap of the tags that tell fresh granules from stale ones.

A pool slot (Slot, aln_host.hip) is reused by whatever call leases it next; `scratch`, `repair`, `cand`, `ctrl`, `tbmap`, `tags`,
`tb` and `walked` are not cleared per launch, the layout inside `scratch` changes from call to call, and the fast batch kernels
tell fresh rows from stale ones by tags whose two counters are narrow: the salt (10 bits, a slot's fast launches; slot_launch
clears `scratch` at its wrap) and the seq (12 bits, a wave's multi-strip passes within one launch; the wave clears its rows, its
bottom-row record and its cooperative record at the wrap).

1. test_every_transition_between_catalogue_entries: the catalogue of tests/call_history.py (one small call per user of a slot)
   run in an order in which every entry directly follows every entry, itself included (K * K + 1 calls), in one fresh process, so
   that the first touch of every buffer is part of it; every call against the oracle.
2. test_salt_wrap[on_a_pooled_slot] / [on_a_staged_batch_private_slot]: three batches of identical shapes and different residues,
   A, B, C, A, .. (1 024 is no multiple of 3: launch n and launch n + 1 024 differ) -- 2 100 calls through align_batch per
   semantics, and 1 100 runs of each of three staged batches, interleaved; every call and every run against the oracle.
3. test_more_than_4096_passes_per_wave_in_one_launch: 22 000 two- and three-strip pairs on four fill waves (ALN_FILL_WGS=1), core
   local 11 / 2 and core global, on the cooperative build (every first pass open, every re-fill shared) and on the lean build;
   every pair against the oracle.

The comparison is call_history.compare everywhere: every field of aln_pair_result but `passes` (diagnostics; with shared passes
it may depend on timing), both strings up to aln_len, D and H where asked for.  No call and no pair is left out.

Every part runs in a child process of its own, one at a time and under its own time limit; when a child dies or times out its
test fails and the tests after it fail without starting anything.

Mutations tried once each on an MI355X (not committed), and what the module said (profiles/r07_call_history.txt):
  (a) slot_launch without `|| s.salt == 0u`                    all five tests pass: NOT caught
  (b) no row clear at (epoch & 0xfff) == 0                     all five tests pass: NOT caught
  (c) scratch_clean stays true after a reallocation            all five tests pass: NOT caught
  (d) no per-pair memset of `granules`, single-pair route      test_every_transition_between_catalogue_entries fails (single_local
                                                               after legacy_local_batch and after fast_local_long: wrong scores)
A stale granule is taken only by a reader that overtakes its writer, and the reader of a strip's rows is claimed after the strip
above it has started and runs at its pace: (a) - (c) change no result in these runs, and the loops were not tuned until they
did.  The same holds for the record that a wave now clears at the pass-count wrap: the commit before that clear passes
test_more_than_4096_passes_per_wave_in_one_launch as well."""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import call_history as ch  # noqa: E402

pytestmark = pytest.mark.gpu
HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "call_history.py")
CHILD_TIMEOUT = 420
PLAN = re.compile(r"aln plan: .* build (\w+)")
_child_lost = []
_expected = {}


def expected_file(tmp_path_factory, key, make, save):
    """The oracle's answers of one part, computed once per session and handed to the child as a file."""
    if key not in _expected:
        path = str(tmp_path_factory.mktemp("call_history") / (key + ".npz"))
        save(path, make())
        _expected[key] = path
    return _expected[key]


def run_child(mode, expected, tmp_path, env):
    assert not _child_lost, "an earlier child process faulted or timed out (%s): nothing more is started" % _child_lost[0]
    report = str(tmp_path / "report.json")
    full = dict(os.environ, ALN_TRACE_PLAN="1")
    for k in ("ALN_COOP_LEAN", "ALN_FILL_WGS", "ALN_COOP_TAIL", "ALN_COOP_DEBUG", "ALN_CHUNK_CELLS", "ALN_CLAIM", "ALN_SINGLE_R"):
        full.pop(k, None)
    full.update(env)
    t0 = time.perf_counter()
    try:
        p = subprocess.run([sys.executable, HELPER, mode, expected, report], env=full, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _child_lost.append("%s: no result within %d s" % (mode, CHILD_TIMEOUT))
        raise
    if p.returncode != 0:
        _child_lost.append("%s: exit status %d" % (mode, p.returncode))
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    with open(report) as f:
        rep = json.load(f)
    print("call history, %s %s: child %.1f s" % (mode, env, time.perf_counter() - t0))
    return rep, PLAN.findall(p.stderr)


def test_every_transition_between_catalogue_entries(orc, tmp_path, tmp_path_factory):
    cat = ch.catalogue()
    path = expected_file(tmp_path_factory, "schedule", lambda: {e.name: e.expected(orc) for e in cat}, ch.save_expected)
    rep, builds = run_child("schedule", path, tmp_path, {})
    seq = ch.schedule(len(cat))
    calls = rep["calls"]
    assert [c["entry"] for c in calls] == [cat[i].name for i in seq] and len(calls) == len(cat) ** 2 + 1
    assert ch.transitions([c["entry"] for c in calls]) == {(a.name, b.name) for a in cat for b in cat}
    per_entry = {}
    for c in calls:
        per_entry.setdefault(c["entry"], []).append(c["seconds"])
    print("seconds per call (median): " + ", ".join("%s %.4f" % (k, float(np.median(v))) for k, v in per_entry.items()))
    wrong = [(c["step"], calls[c["step"] - 1]["entry"] if c["step"] else None, c["entry"], c["diff"]) for c in calls if c["diff"] is not None]
    assert not wrong, "%d of %d calls differ from the oracle; (step, after, entry, what): %s" % (len(wrong), len(calls), wrong[:8])
    off_route = [(c["step"], c["entry"]) for c in calls if not c["routed"]]
    assert not off_route, off_route[:8]
    assert "coop" in builds, "no call of the schedule shared passes"


@pytest.mark.parametrize("mode", ["wrap_pooled", "wrap_staged"], ids=["on_a_pooled_slot", "on_a_staged_batch_private_slot"])
def test_salt_wrap(orc, tmp_path, tmp_path_factory, mode):
    path = expected_file(tmp_path_factory, "wrap", lambda: ch.wrap_expected(orc), ch.flat_save)
    rep, builds = run_child(mode, path, tmp_path, {})
    assert set(rep) == {name for name, _ in ch.WRAP_SEMS}
    launches = 0
    for name, r in rep.items():
        print("call history, %s %s: %s" % (mode, name, {k: v for k, v in r.items() if k != "first_bad"}))
        if mode == "wrap_pooled":
            assert r["calls"] >= 2 * 1024 + 50
            launches += r["calls"]
        else:
            assert r["runs_each"] >= 1024 + 50 and r["batches"] == 3
            launches += r["runs_each"] * r["batches"]
        assert r["bad"] == 0, "%s: %d launches differ from the oracle; (launch, batch, what): %s" % (name, r["bad"], r["first_bad"])
    # (a call through align_batch is planned every time, a staged batch once)
    planned = launches if mode == "wrap_pooled" else 3 * len(ch.WRAP_SEMS)
    assert len(builds) == planned and set(builds) == {"coop"}, (len(builds), planned, set(builds))


@pytest.mark.parametrize("lean", [0, 1], ids=["cooperative", "lean"])
def test_more_than_4096_passes_per_wave_in_one_launch(orc, tmp_path, tmp_path_factory, lean):
    path = expected_file(tmp_path_factory, "passes", lambda: {name: ch.pass_expected(orc, sem) for name, sem in ch.WRAP_SEMS}, ch.flat_save)
    env = dict(ALN_FILL_WGS="1", ALN_COOP_LEAN=str(lean))
    if not lean:
        env.update(ALN_COOP_TAIL=str(10 * ch.PASS_PAIRS), ALN_COOP_DEBUG="8")      # every first pass open, every re-fill shared
    rep, builds = run_child("passes", path, tmp_path, env)
    assert builds == ["lean" if lean else "coop"] * len(ch.WRAP_SEMS), builds
    assert set(rep) == {name for name, _ in ch.WRAP_SEMS}
    for name, r in rep.items():
        print("call history, passes lean=%d %s: %s" % (lean, name, r))
        assert r["pairs"] == ch.PASS_PAIRS and r["pairs"] / 4 > 4096
        assert r["bad"] == 0 and r["diff"] is None, "%s: %d of %d pairs differ from the oracle, first %s (%s)" % (
            name, r["bad"], r["pairs"], r["first_bad"], r["diff"])
        assert r["routed"], name
