"""A resident sequence set on every fill route of chunk_plan: the route is proven by the `aln route:` line of ALN_TRACE_PLAN (and,
where summaries come back, by the flags word), the answers are compared with the CPU oracle bit for bit.

A set's passes reach the fill and traceback kernels by a road of their own: score, best and candidate passes expand their
descriptors on the device and launch the pairs routed off the batch kernel from the host's copy (chunk_resident), re-uploading the
queue only when it is not the identity; a held pass runs on the set's private slot and copies the strings into the held store
behind the launches, the overlapped traceback's second stream included.  The blocks of tests/route_cases.py put one set on

  duo            3600 short pairs, core global 4 / 4         two pairs per wave (aln_fill_duo_kernel), score and held pass
  overlap        4186 short pairs, held                      walk waves beside the fill, in front of the held store's copy
  single_alone   600 x 640                                   the single-pair route by the time rule alone
  single_mixed   {520, a 600 ending in code 24, 40} x {640, 2600, 30}, core local and core global
                                                             big pairs on the single-pair route (2600 rows: R = 2), two of them
                                                             failing there with ALN_ERR_CODE_OUT_OF_RANGE, the queue not the identity
  coop           the 21 pairs of seven multi-strip sequences cooperative passes
  wg_real        {300, 600} x {130, 640}, real-valued        one workgroup per pair, f64
  wg_mixed       {300} x {130, 40, 1100}, real-valued        two on a workgroup each, 40 rows with the batch kernel
  wg_int         {300, 520} x {130}, an entry of 33          one workgroup per pair, integer kernels off the fast path

a. every block, every pass (score; hits at -inf with strings; best k = 2 on the rectangles; the same three over the candidate list
   of a prefilter that keeps every pair) against the oracle, every planned chunk's route line against route_cases.plan;
b. the held pass of the eight blocks in the order of call_history.schedule(8) on one set -- 65 calls, every ordered pair of routes
   once on the one private slot -- and again with a score pass of the previous block between two calls;
c. overlap, duo, coop and wg_real with their machinery switched off: the route line shows it gone, the bytes are those of (a).

Everything runs in child processes started fresh (the knobs are read from the environment; ALN_TRACE_PLAN once per process);
after a child that died or timed out nothing more is started.  The failing pairs are inputs the reference rejects, no device
faults.  best is refused on an upper block (overlap, coop), so those have no best pass."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import call_history as ch  # noqa: E402
import route_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu
HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "route_cases.py")
CHILD_TIMEOUT = 300
KNOBS = ("ALN_NO_DUO", "ALN_NO_COOP", "ALN_NO_WGPIPE", "ALN_TB_OVERLAP", "ALN_CHUNK_CELLS", "ALN_COOP_LEAN", "ALN_SINGLE_R", "ALN_NO_SINGLE",
         "ALN_WG_R", "ALN_FILL_WGS", "ALN_COOP_TAIL", "ALN_CHAIN_WGS", "ALN_CLAIM", "ALN_NO_DYADIC")
_child_lost = []
_cache = {}


def wants(orc, tmp_path_factory):
    """The oracle's answers of every block, computed once per session and handed to the children as a file."""
    if "wants" not in _cache:
        t0 = time.perf_counter()
        w = {b.name: rc.expected(orc, b, threads=16) for b in rc.blocks()}
        path = str(tmp_path_factory.mktemp("set_routes") / "expected.npz")
        ch.save_expected(path, w)
        _cache["wants"] = (w, path)
        print("set routes: oracle %.1f s" % (time.perf_counter() - t0))
    return _cache["wants"]


def run_child(mode, expected, tmp_path, extra=None, only=None):
    assert not _child_lost, "an earlier child process faulted or timed out (%s): nothing more is started" % _child_lost[0]
    report = str(tmp_path / "report.json")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(rc.CHILD_ENV)
    env.update(extra or {})
    cmd = [sys.executable, HELPER, mode, expected, report] + ([only] if only else [])
    t0 = time.perf_counter()
    try:
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _child_lost.append("%s: no result within %d s" % (mode, CHILD_TIMEOUT))
        raise
    if p.returncode != 0:
        _child_lost.append("%s: exit status %d" % (mode, p.returncode))
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    with open(report) as f:
        rep = json.load(f)
    calls = rep["calls"]
    print("set routes, %s %s %s: child %.1f s, %d calls, the calls themselves %.2f s" % (
        mode, only or "", extra or "", time.perf_counter() - t0, len(calls), sum(c["seconds"] for c in calls)))
    return calls, rc.cut_by_call(p.stderr)


def planned(b, want, kind_of_pass, env):
    """The route lines a call must print, and (held calls) the plan of the held pass: a pass over every pair of the block without
    directions, then -- hits, best -- the held pass over the pairs it keeps."""
    L = rc.set_lengths()
    q, t = b.pairs()
    _, dele, ext, kind = rc.schemes()[b.scheme]
    lines = [rc.plan(L[q], L[t], kind, b.local(), dele, ext, False, env)]
    if kind_of_pass in ("score", "cand_score", "between"):
        return lines, None
    keep = want["index"].astype(np.int64)
    if kind_of_pass in ("best", "cand_best"):
        keep = rc.best_rule(q, t, want["pair_f"], want["pair_status"], b.tn, 2)
    held = rc.plan(L[q[keep]], L[t[keep]], kind, b.local(), dele, ext, True, env)
    return lines + [held], held


def check_call(c, routes, b, want, kind_of_pass, env):
    assert c["diff"] is None, (c["label"], c["diff"])
    lines, held = planned(b, want, kind_of_pass, env)
    got = routes[c["label"]]
    print("%-32s %s" % (c["label"], "; ".join(" ".join("%s %s" % kv for kv in g.items()) for g in got)))
    assert got == [rc.line_of(p) for p in lines], (c["label"], got, [rc.line_of(p) for p in lines])
    if held is not None:
        mask, val = rc.want_flags(held, held["kernels"])
        flags = np.asarray(c["flags"], dtype=np.uint32)
        assert len(flags) == held["pairs"] and np.array_equal(flags & mask, val), (c["label"], flags.tolist(), val.tolist())


def passes_of(b, candidates=True):
    out = ["score", "hits"] + ([] if b.upper else ["best"])
    if candidates:
        out += ["cand_score"] + ([] if b.name in ("duo", "overlap") else ["cand_hits"] + ([] if b.upper else ["cand_best"]))
    return out


def all_passes(orc, tmp_path_factory):
    """(a)'s child, once per session: (c) compares its own bytes with it."""
    if "passes" not in _cache:
        w, path = wants(orc, tmp_path_factory)
        _cache["passes"] = run_child("passes", path, tmp_path_factory.mktemp("set_routes_a"))
    return _cache["passes"]


def test_every_block_every_pass_against_the_oracle(orc, tmp_path_factory):
    w, _ = wants(orc, tmp_path_factory)
    calls, routes = all_passes(orc, tmp_path_factory)
    by_label = {c["label"]: c for c in calls}
    assert list(by_label) == [b.name + "/" + p for b in rc.blocks() for p in passes_of(b)]
    for b in rc.blocks():
        for p in passes_of(b):
            check_call(by_label[b.name + "/" + p], routes, b, w[b.name], p, rc.CHILD_ENV)
        # the table: the held pass over every pair that succeeded shows the block's route
        held = routes[b.name + "/hits"][1]
        assert {k: held[k] for k in b.want} == b.want, (b.name, held)
        # a pass over the candidate list leaves the bytes of the pass over the block
        for p in passes_of(b):
            if p.startswith("cand_"):
                assert by_label[b.name + "/" + p]["digest"] == by_label[b.name + "/" + p[5:]]["digest"], (b.name, p)
    # what the rows of the table say beyond the held pass
    assert routes["duo/score"][0]["duo"] == 1 and routes["overlap/score"][0]["overlap"] == 0 and routes["coop/score"][0]["share"] == "coop"
    for name in ("single_mixed", "single_mixed_global"):
        sc = routes[name + "/score"][0]
        assert (sc["single"], sc["small"], sc["pairs"]) == (4, 5, 9)                      # the failing big pairs are routed single as well
        assert (w[name]["pair_status"] == rc.ERR_CODE_OUT_OF_RANGE).sum() == 3
    for name, bit in (("single_alone", rc.FLAG_SINGLE), ("wg_real", rc.FLAG_WORKGROUP), ("wg_int", rc.FLAG_WORKGROUP | rc.FLAG_INTEGER)):
        assert all(f & bit == bit for f in by_label[name + "/hits"]["flags"]), name
    assert not any(f & rc.FLAG_INTEGER for f in by_label["wg_real/hits"]["flags"])
    assert not any(f & rc.FLAG_FAST for f in by_label["wg_int/hits"]["flags"])
    assert sorted(f & rc.FLAG_SINGLE for f in by_label["single_mixed/hits"]["flags"]) == [0, 0, 0, 0, 2, 2]
    assert sorted(f & rc.FLAG_WORKGROUP for f in by_label["wg_mixed/hits"]["flags"]) == [0, 4, 4]


@pytest.mark.parametrize("between", [False, True], ids=["held_after_held", "a_score_pass_between"])
def test_every_transition_on_the_private_slot(orc, tmp_path, tmp_path_factory, between):
    w, path = wants(orc, tmp_path_factory)
    calls, routes = run_child("schedule_between" if between else "schedule", path, tmp_path)
    names = rc.schedule_names()
    held = [c for c in calls if c["label"].endswith("/hits")]
    assert [c["label"] for c in held] == ["%d/%s/hits" % (i, n) for i, n in enumerate(names)] and len(held) == 65
    assert ch.transitions([c["label"].split("/")[1] for c in held]) == {(a.name, b.name) for a in rc.blocks()[:8] for b in rc.blocks()[:8]}
    assert len(calls) == (129 if between else 65)
    wrong = [(c["label"], c["diff"]) for c in calls if c["diff"] is not None]
    assert not wrong, "%d of %d calls differ from the oracle: %s" % (len(wrong), len(calls), wrong[:8])
    for c in calls:
        step, name, kind = c["label"].split("/")
        check_call(c, routes, rc.block(name), w[name], kind, rc.CHILD_ENV)
    if between:
        assert [c["label"].split("/")[1] for c in calls if c["label"].endswith("/between")] == names[:-1]


OFF = [("overlap", {"ALN_TB_OVERLAP": "0"}, "overlap", 0), ("duo", {"ALN_NO_DUO": "1"}, "duo", 0), ("coop", {"ALN_NO_COOP": "1"}, "share", "none"),
       ("wg_real", {"ALN_NO_WGPIPE": "1"}, "wg", 0)]


@pytest.mark.parametrize("name,knob,key,gone", OFF, ids=[o[0] for o in OFF])
def test_the_same_bytes_with_the_machinery_off(orc, tmp_path, tmp_path_factory, name, knob, key, gone):
    w, path = wants(orc, tmp_path_factory)
    on = {c["label"]: c for c in all_passes(orc, tmp_path_factory)[0]}
    on_routes = all_passes(orc, tmp_path_factory)[1]
    calls, routes = run_child("passes", path, tmp_path, knob, only=name)
    b, env = rc.block(name), dict(rc.CHILD_ENV, **knob)
    assert [c["label"] for c in calls] == [name + "/" + p for p in passes_of(b, False)]
    for c in calls:
        check_call(c, routes, b, w[name], c["label"].split("/")[1], env)
        assert c["digest"] == on[c["label"]]["digest"], c["label"]
    assert on_routes[name + "/hits"][1][key] == b.want[key] != gone and routes[name + "/hits"][1][key] == gone
    assert all(line[key] == gone for label in routes for line in routes[label])
