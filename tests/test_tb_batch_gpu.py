"""The batch traceback (aln_traceback_kernel, aln_traceback_wave_kernel, aln_traceback_overlap_kernel, aln_traceback_expand_kernel)
on the constructed paths of tests/tb_batch_cases.py: tag counts around the 64-tag flush and the 128-position expand rounds, border
runs, gap runs that carry the path out of the wave walk's three-quad window either way, strip changes with every R of a last strip,
Top runs in a lane's last block, thin pairs; every reader and writer of the direction store (batch fast kernel, aln_fill_f64_kernel,
the generic integer kernel, the row-major fallback, the two-pairs-per-wave kernel's regions, PWM windows).

Every expectation is the CPU oracle's; tests/test_tb_batch_model_cpu.py has shown on the CPU that each case's path lies where its aim
says.  One pair per call compares the whole D as well (aln_unpack_directions_kernel reads the store cell by cell: a D that agrees and
a string that does not is the walk's fault).  The batches whose route has to be proved run in a child process whose `aln route:` line
(ALN_TRACE_PLAN) is asserted."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tb_batch_cases as tc  # noqa: E402
from route_cases import ROUTE, ROUTE_KEYS  # noqa: E402
from aligner_amd import runtime  # noqa: E402
from aligner_amd.batch import PairBatch, align_batch  # noqa: E402
from aligner_amd.pwm import align_window_offsets  # noqa: E402

pytestmark = pytest.mark.gpu
HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tb_batch_cases.py")
CHILD_TIMEOUT = 120
KNOBS = ("ALN_TB_WAVE", "ALN_TB_OVERLAP", "ALN_TB_OVERLAP_ANY", "ALN_TB_WAIT_US", "ALN_NO_SINGLE", "ALN_NO_WGPIPE", "ALN_NO_DUO", "ALN_NO_COOP",
         "ALN_TRACE_PLAN", "ALN_BIG_TO_SINGLE")
CASES = tc.cases()
GROUPS = sorted({c.group for c in CASES})
_refs = {}
_child_lost = []


def ref_of(orc, case, kind="int"):
    """The oracle's answer with its D, once per session and left unchanged."""
    key = (case.id, kind)
    if key not in _refs:
        ref = tc.oracle(orc, case, kind, want_matrices=True)
        assert ref["status"] == 0, key
        ref.pop("H")
        _refs[key] = ref
    return _refs[key]


def check(res, qa, ta, D, ref, where):
    assert res.status == 0, where
    assert (res.score, res.f) == (ref["score"], ref["f"]), where
    assert (res.end_y, res.end_x) == ref["end"], where + ((res.end_y, res.end_x), ref["end"])
    if D is not None:
        bad = np.argwhere(D != ref["D"])
        assert len(bad) == 0, where + ("D differs in %d cells, first at (y, x) = %s" % (len(bad), bad[0] if len(bad) else None),)
    assert (res.start_y, res.start_x) == ref["start"], where + ((res.start_y, res.start_x), ref["start"])
    assert res.aln_len == len(ref["qa"]), where + (res.aln_len, len(ref["qa"]))
    assert qa.tolist() == ref["qa"].tolist() and ta.tolist() == ref["ta"].tolist(), where + ("strings",)


def run_pair(orc, monkeypatch, case, kind, wave, **kw):
    q, t = case.seqs()
    S, dele, ext = tc.scheme(kind)
    ref = ref_of(orc, case, kind)
    monkeypatch.setenv("ALN_NO_SINGLE", "1")
    monkeypatch.setenv("ALN_NO_WGPIPE", "1")        # the generic kernels write the skewed layout the batch walks read
    monkeypatch.setenv("ALN_TB_WAVE", str(wave))
    res, qa, ta, D, _ = runtime.align_pair(case.sem, q, t, dele, ext, S, want_directions=True, **kw)
    where = (case.id, kind, "wave" if wave else "lane", hex(res.flags), hex(res.passes))
    if kw.get("force_serial"):
        assert res.passes & 0x80, where                              # row-major
    elif kind == "int":
        assert (res.flags & 0xe) == 8, where                         # the batch fast kernel
    else:
        assert (res.flags & 0xe) == 0 and (res.flags & 1) == (1 if kind == "off" else 0), where      # aln_fill_f64_kernel / the generic integer kernel
    check(res, qa, ta, D, ref, where)


@pytest.mark.parametrize("wave", [1, 0], ids=["wave", "lane"])
@pytest.mark.parametrize("group", GROUPS)
def test_fast_kernel_pairs(orc, monkeypatch, group, wave):
    t0 = time.perf_counter()
    sel = [c for c in CASES if c.group == group]
    for c in sel:
        run_pair(orc, monkeypatch, c, "int", wave)
    print("%s: %d cases, %.1f s" % (group, len(sel), time.perf_counter() - t0))


@pytest.mark.parametrize("wave", [1, 0], ids=["wave", "lane"])
@pytest.mark.parametrize("kind", ["real", "off", "serial"])
def test_subset_on_the_other_writers(orc, monkeypatch, kind, wave):
    sel = [c for c in CASES if c.subset and (kind == "serial" or kind in tc.kinds_of(c))]
    legacy_only = {"end_row"} | ({"border", "interior"} if kind == "real" else set())      # (the legacy semantics are integer only)
    assert {n for c in sel for n in c.aim} >= {n for c in CASES for n in c.aim} - legacy_only
    for c in sel:
        if kind == "serial":
            run_pair(orc, monkeypatch, c, "int", wave, force_serial=True)
        else:
            run_pair(orc, monkeypatch, c, kind, wave)


def _batch_equal(a, b, n):
    for f in ("status", "score", "f", "end_y", "end_x", "start_y", "start_x", "aln_len"):
        assert (a.results[f] == b.results[f]).all(), f
    for i in range(n):
        (qa, ta), (qb, tb) = a.aligned(i), b.aligned(i)
        assert (qa == qb).all() and (ta == tb).all(), i


@pytest.mark.parametrize("sem", [s for _, s in tc.SEMS], ids=[n for n, _ in tc.SEMS])
def test_all_cases_as_one_batch(orc, monkeypatch, sem):
    """Neighbouring pairs' tag and string regions at the cap N + M + 2: every case of one semantics in one call, both walks."""
    sel = [c for c in CASES if c.sem == sem]
    pb = PairBatch.from_pairs([c.seqs() for c in sel])
    S, dele, ext = tc.scheme("int")
    monkeypatch.setenv("ALN_NO_SINGLE", "1")
    monkeypatch.setenv("ALN_TB_WAVE", "1")
    wave = align_batch(pb, sem, dele, ext, S)
    monkeypatch.setenv("ALN_TB_WAVE", "0")
    lane = align_batch(pb, sem, dele, ext, S)
    _batch_equal(wave, lane, len(pb))
    ref, tb, tb_off = orc.align_batch(sem, pb.seqs, pb.q_off, pb.q_len, pb.t_off, pb.t_len, dele, ext, S, n_threads=8)
    for i, c in enumerate(sel):
        r, g = ref[i], wave.results[i]
        assert int(g["status"]) == r.status == 0, c.id
        assert (g["score"], g["f"], g["end_y"], g["end_x"], g["start_y"], g["start_x"], g["aln_len"]) == \
            (r.score, r.f, r.end_y, r.end_x, r.start_y, r.start_x, r.aln_len), c.id
        cap, o = int(pb.q_len[i] + pb.t_len[i]) + 2, int(tb_off[i])
        qa, ta = wave.aligned(i)
        assert (qa == tb[o:o + r.aln_len]).all() and (ta == tb[o + cap:o + cap + r.aln_len]).all(), c.id


# ---- batches in a child process
def run_child(mode, env_extra, tmp_path, name):
    assert not _child_lost, "an earlier child process faulted or timed out (%s): nothing more is started" % _child_lost[0]
    report = str(tmp_path / (name + ".npz"))
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_extra, ALN_TRACE_PLAN="1", ALN_NO_SINGLE="1")
    try:
        p = subprocess.run([sys.executable, HELPER, mode, report], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _child_lost.append("no result within %d s" % CHILD_TIMEOUT)
        raise
    if p.returncode != 0:
        _child_lost.append("exit status %d" % p.returncode)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    routes = [dict(zip(ROUTE_KEYS, [int(v) for v in m.groups()[:6]] + list(m.groups()[6:]))) for m in ROUTE.finditer(p.stderr)]
    routes = [r for r in routes if r["pairs"] > 1]           # (a process's first call also plans the pair the context warms up with)
    with np.load(report) as z:
        return routes, dict(results=z["results"], strings=z["strings"], off=z["off"])


def _strings(got, i):
    o = got["off"]
    s = got["strings"][o[i]:o[i + 1]]
    return s[:len(s) // 2], s[len(s) // 2:]


def _same(a, b):
    for f in ("status", "score", "f", "end_y", "end_x", "start_y", "start_x", "aln_len"):
        assert (a["results"][f] == b["results"][f]).all(), f
    assert (a["off"] == b["off"]).all() and (a["strings"] == b["strings"]).all(), "strings"


def _check_against_oracle(orc, got, i, q, t, sem, S, dele, ext, where):
    ref = orc.align(sem, q, t, dele, ext, S)
    g = got["results"][i]
    assert int(g["status"]) == ref["status"] == 0, where
    assert (g["score"], g["f"], (g["end_y"], g["end_x"]), (g["start_y"], g["start_x"]), g["aln_len"]) == \
        (ref["score"], ref["f"], ref["end"], ref["start"], len(ref["qa"])), where
    qa, ta = _strings(got, i)
    assert qa.tolist() == ref["qa"].tolist() and ta.tolist() == ref["ta"].tolist(), where


def test_two_pairs_per_wave_batches_hold_every_case():
    held = {c.id for mode in tc.UBATCH_MODES for c in tc.batch_of(mode)[1].values()}
    assert held == {c.id for c in tc.ubatch_cases()} and len(held) == 15


@pytest.mark.parametrize("mode", tc.UBATCH_MODES)
def test_two_pairs_per_wave_regions(orc, tmp_path, mode):
    """ALN_LAYOUT_UBATCH as aln_fill_duo_kernel writes it (32 lanes a pair, R = ceil(rows / 32)), read by both walks.  Each case
    stands twice; tc.duo_halves restates the work queue's order (cost, then position) and the kernel's split of an item, and by it one
    copy is filled by lanes 0 .. 31 and the other by lanes 32 .. 63.  That the kernel keeps to that order is supposed, not observed:
    the route line says only that the kernel ran."""
    pairs, at, sem, (S, dele, ext) = tc.batch_of(mode)
    half = tc.duo_halves(pairs)
    assert len(pairs) >= 3100 and all({half[p] for p, c2 in at.items() if c2 is c} == {0, 1} for c in at.values())
    routes, lane = run_child(mode, {}, tmp_path, "lane")
    assert [r["duo"] for r in routes] == [1], routes
    routes, wave = run_child(mode, {"ALN_TB_WAVE": "1"}, tmp_path, "wave")
    assert [r["duo"] for r in routes] == [1], routes
    _same(lane, wave)
    for pos, c in at.items():
        _check_against_oracle(orc, lane, pos, *pairs[pos], sem, S, dele, ext, (mode, c.id, pos))
    for pos in range(0, len(pairs), 97):
        _check_against_oracle(orc, lane, pos, *pairs[pos], sem, S, dele, ext, (mode, "filler", pos))


def test_overlapped_walk(orc, tmp_path):
    """The walk kernel beside the fill (tb_walk_pair as the body of aln_traceback_overlap_kernel), the ordinary walk picking up what it
    gave up on (ALN_TB_WAIT_US=0), and no overlap at all: the same batch three times."""
    pairs, at, sem, (S, dele, ext) = tc.batch_of("overlap")
    assert len(pairs) >= 4096 + len(at)
    routes, over = run_child("overlap", {"ALN_TB_OVERLAP_ANY": "1"}, tmp_path, "over")
    assert [r["overlap"] for r in routes] == [1], routes
    routes, gave_up = run_child("overlap", {"ALN_TB_OVERLAP_ANY": "1", "ALN_TB_WAIT_US": "0"}, tmp_path, "gave_up")
    assert [r["overlap"] for r in routes] == [1], routes
    routes, off = run_child("overlap", {"ALN_TB_OVERLAP_ANY": "1", "ALN_TB_OVERLAP": "0"}, tmp_path, "off")
    assert [r["overlap"] for r in routes] == [0], routes
    _same(over, gave_up)
    _same(over, off)
    for pos, c in at.items():
        _check_against_oracle(orc, over, pos, *pairs[pos], sem, S, dele, ext, ("overlap", c.id, pos))


@pytest.mark.parametrize("real", [True, False], ids=["real", "int"])
def test_pwm_windows(orc, monkeypatch, real):
    """No seed pair, column numbers in place of the query string; path lengths on both sides of 64 and 128."""
    pwm, dele, ext, wins = tc.pwm_cases(real)
    seq = np.concatenate([w for _, w in wins])
    lens = np.array([len(w) for _, w in wins], dtype=np.uint64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    for wave in (1, 0):
        monkeypatch.setenv("ALN_TB_WAVE", str(wave))
        res, alns = align_window_offsets(seq, starts, lens, dele, ext, pwm)
        for i, (name, w) in enumerate(wins):
            ref = orc.align_pwm(w, dele, ext, pwm)
            r = res[i]
            where = (name, real, wave)
            assert int(r["status"]) == ref["status"] == 0, where
            assert (r["f"], (r["end_y"], r["end_x"]), (r["start_y"], r["start_x"]), r["aln_len"]) == \
                (ref["f"], ref["end"], ref["start"], len(ref["numbered"])), where
            assert alns[i].numbered.tolist() == ref["numbered"].tolist() and alns[i].query.tolist() == ref["qal"].tolist(), where
