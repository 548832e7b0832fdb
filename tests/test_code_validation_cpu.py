"""The catalogue of tests/code_validation_cases.py, certified without a GPU.

a. The oracle refuses every bad line with ERR_CODE_OUT_OF_RANGE and aligns every twin, every legal non-square line and every neighbour,
   each with an alignment worth the name; every sequence stands between two guard bytes; the bytes a query check would read under PWM
   scoring hold a code the PWM has no column for.
b. The header's own plan (tests/plan_rules_driver.cpp over aln_plan_rules.h) puts every batch where route_cases.plan() and the route's
   table say, every line on its route's list, and orders the queue of the two-pairs-per-wave batches as queue_order() does, so that the
   lines run in the halves they are meant for.
c. Every stride edge is there for every route that can hold it.
d. The catalogue's checker passes a backend that is right by construction (the oracle's answers behind the restated scans) and reports
   each planted fault of the scan by name, with the lines that caught it."""
import numpy as np
import pytest

import code_validation_cases as cv
import plan_cases as pc
import route_cases as rc
from test_plan_rules_cpu import driver  # noqa: F401  (the fixture that builds the plan-rule driver)

ROUTES = [r.name for r in cv.routes()]
_wants = {}


def wants(orc, rt):
    if rt.name not in _wants:
        _wants[rt.name] = [cv.expected(orc, b) for b in cv.batches(rt)]
    return _wants[rt.name]


@pytest.mark.parametrize("name", ROUTES)
def test_the_oracle_certifies_every_line(orc, name):
    rt = cv.route(name)
    n_bad = n_twin = 0
    for b, want in zip(cv.batches(rt), wants(orc, rt)):
        assert b.guarded(), b.name
        rows, cols = b.dims()
        for i in range(len(b)):
            ln = b.lines.get(i)
            if ln is not None and ln.bad:
                assert want["status"][i] == cv.REFUSED, ln.name
                side = b.pairs[i][0] if ln.side == "q" else b.pairs[i][1]
                dim = cols if ln.side == "q" else rows
                assert side[ln.pos] == ln.value >= dim and (np.delete(side, ln.pos) < dim).all(), ln.name
                n_bad += 1
                continue
            assert want["status"][i] == cv.OK, (b.name, i)
            # an alignment worth the name: a good pair that scores nothing proves little
            # (core global: f is 0 by definition, the score is the corner cell's and the path spans both sequences)
            worth = want["f"][i] > 0 if rt.local else want["score"][i] != 0 and want["aln_len"][i] >= max(b.q_len[i], b.t_len[i])
            assert worth and want["aln_len"][i] >= min(4, int(b.t_len[i])), (b.name, i, want["f"][i], want["score"][i], want["aln_len"][i])
            if ln is not None:
                n_twin += 1
        assert set(b.lines) and all(0 < i < len(b) - 1 for i in b.lines) or rt.kind == "pair" or rt.fillers, b.name
        if rt.pwm():                                             # what a query check would read: the first N bytes that go up
            lo = int(b.t_off.min())
            assert b.seqs[lo:lo + cols].max() >= cols, b.name
    # every bad line of the positions has its twin; the non-square lines come as legal / illegal
    tw = {ln.name for b in cv.batches(rt) for ln in b.lines.values()}
    for t in tw:
        if t.endswith("/edge") or t.endswith("/255"):
            assert t + "/twin" in tw, t
    assert n_bad >= 8 and n_twin >= 8, (n_bad, n_twin)
    if not rt.pwm():
        for shape in ("tall", "wide"):
            kinds = sorted(t.rsplit("/", 1)[1] + t.split("/")[2][0] for t in tw if "/%s/" % shape in t)
            assert kinds == (["illegalq", "legalt"] if shape == "tall" else ["illegalt", "legalq"]), (shape, kinds)
    print("%s: %d batches, %d bad lines, %d lines that must succeed" % (name, len(cv.batches(rt)), n_bad, n_twin))


@pytest.mark.parametrize("name", ROUTES)
def test_the_headers_plan_puts_every_line_on_its_route(driver, name):  # noqa: F811
    rt = cv.route(name)
    bs = cv.batches(rt)
    out, lists = driver([(cv.plan_case(b), cv.plan_facts(b)) for b in bs], lists=True)
    for b in bs:
        o, l = out[b.name], lists[b.name]
        got = dict(pairs=o["n"], small=o["n_small"], single=o["n_single"], wg=o["n_wg"], duo=int(o["duo_qo"] != 0), overlap=o["overlap"],
                   share="coop" if o["coop"] else "lean" if o["coop_lean"] else "none", kernels=cv.planned(b)["kernels"])
        assert cv.route_problems(b, got) == [], b.name
        p = cv.planned(b)
        assert l["single"] == list(np.flatnonzero(p["single_mask"])) and l["wg"] == list(np.flatnonzero(p["wg_mask"])), b.name
        for i in b.lines:
            assert (i in l[rt.on]) if rt.on != "small" else (i in l["order"]), (b.name, i)
        if rt.on == "wg":                                        # the stride of the site: the threads the launcher starts
            R = dict(zip(l["wg"], l["wg_r"]))
            for i, ln in b.lines.items():
                M = int(b.t_len[i])
                assert cv.wg_threads(M) == 64 * ((M + 64 * R[i] - 1) // (64 * R[i])) == (rt.sq if ln.side == "q" else rt.st), ln.name
        if rt.fillers:
            assert l["order"] == cv.queue_order(b.columns(), b.t_len), b.name
            hv = cv.halves(b)
            for i, ln in b.lines.items():
                assert ln.half is None or hv[i][1] == ln.half, (ln.name, hv[i])   # (None: a non-square line, either half)


def test_the_two_halves_of_a_wave_meet_as_intended():
    rt = cv.route("duo")
    by = {b.name.split("/")[1]: b for b in cv.batches(rt)}

    def partners(b):
        """[(bad?, bad?)] per queue item that holds a line"""
        hv, items = cv.halves(b), {}
        for i, (item, half) in hv.items():
            items.setdefault(item, [None, None])[half] = i
        return [tuple(None if i is None else (i in b.lines and b.lines[i].bad) for i in items[it]) for it in sorted({hv[i][0] for i in b.lines})]
    assert partners(by["bad_good"]) == [(True, False)] and partners(by["good_bad"]) == [(False, True)]
    assert partners(by["bad_bad"]) == [(True, True), (False, False)]
    assert partners(by["odd"])[-1] == (True, None) and len(by["odd"]) % 2 == 1
    pos = partners(by["positions"])
    assert set(pos) == {(True, False), (False, True)} and len(pos) == 16
    for b in by.values():                                        # more pairs than 12 per CU: what aln_plan_duo asks for
        assert len(b) > 12 * rc.CUS and max(b.t_len) <= 256


@pytest.mark.parametrize("name", ROUTES)
def test_every_stride_edge_is_there(name):
    rt = cv.route(name)
    have = {(ln.side, ln.pos, "edge" if ln.name.endswith("/edge") else "255") for b in cv.batches(rt) for ln in b.lines.values()
            if ln.bad and "/tall/" not in ln.name and "/wide/" not in ln.name}
    for side in ("q", "t"):
        if side == "q" and rt.pwm():
            continue                                             # EXCLUDED: no query sequence
        (N, M), s = (rt.q_shape, rt.sq) if side == "q" else (rt.t_shape, rt.st)
        L = N if side == "q" else M
        want = {0, s - 1, s, L - 1}
        assert L % s != 0 and L - 1 >= (L // s) * s              # the last index lies in a partial stride
        if side == "t" and rt.name in ("lean", "coop", "single_pair", "single_batch"):
            want |= {511, 512}
        for p in want:
            for v in ("edge", "255"):
                assert (side, p, v) in have, (name, side, p, v)
    strides = dict(duo=32, wg_int=None, wg_real=None, pwm_wg=None)
    s = strides.get(name, 64)
    if s is None:
        assert rt.st == cv.wg_threads(rt.t_shape[1]) and (rt.pwm() or rt.sq == cv.wg_threads(rt.q_shape[1]))
    else:
        assert rt.st == s and (rt.pwm() or rt.sq == s)


@pytest.mark.parametrize("name", ROUTES)
def test_the_checker_passes_a_backend_that_is_right(orc, name):
    rt = cv.route(name)
    for b, want in zip(cv.batches(rt), wants(orc, rt)):
        assert cv.check(b, cv.fake_answer(b, want), want) == [], b.name


# which routes can show a fault at all
APPLIES = dict(both_sides_against_cols=lambda rt: not rt.pwm(), query_checked_under_pwm=lambda rt: rt.pwm(),
               duo_verdict_from_whole_ballot=lambda rt: bool(rt.fillers))


@pytest.mark.parametrize("fault", cv.FAULTS)
def test_every_planted_fault_is_caught_by_a_named_line(orc, fault):
    caught_any = False
    for rt in cv.routes():
        if not APPLIES.get(fault, lambda rt: True)(rt):
            continue
        caught = []
        for b, want in zip(cv.batches(rt), wants(orc, rt)):
            caught += [n for n, _ in cv.check(b, cv.fake_answer(b, want, fault), want)]
        print("fault %s on %s: caught by %d lines, first %s" % (fault, rt.name, len(caught), caught[:4]))
        assert caught, "fault %s on route %s: no line notices it" % (fault, rt.name)
        caught_any = True
    assert caught_any


def test_counts_per_route():
    """the table of DESIGN.md"""
    for rt in cv.routes():
        bs = cv.batches(rt)
        lines = [ln for b in bs for ln in b.lines.values()]
        print("%-13s batches %3d pairs %5d lines %3d refused %3d" % (rt.name, len(bs), sum(len(b) for b in bs), len(lines), sum(ln.bad for ln in lines)))
    assert len(cv.SITES) == 6
