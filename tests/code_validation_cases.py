"""Helpers of the residue-code validation tests (tests/test_code_validation_*.py).  Not a test module (no test_ prefix).

A residue code outside the scoring matrix is a per-pair status (ALN_ERR_CODE_OUT_OF_RANGE); the check is written six times in
aligner_amd/csrc/aln_kernels.hip (SITES), each with its own indexing.  This catalogue puts one offending byte at every edge of every
site's scan:

* routes(): one entry per validation site and kernel build, at the smallest shape that reaches it, with the knobs that select it.  What
  a route's `aln route:` line (ALN_TRACE_PLAN) must say comes from route_cases.plan(); tests/test_code_validation_cpu.py runs every
  batch through the header's own plan (tests/plan_rules_driver.cpp) as well.
* batches(route): small batches.  A LINE is one pair with one special byte: `bad` lines hold `cols` (query side) or `rows` (target side)
  exactly, or 255, at one index; every bad line has a TWIN with `cols - 1` / `rows - 1` at the same index, which must succeed and equal
  the oracle.  Lines sit between good pairs; every sequence has a byte of 255 directly before and directly after it in the packed
  buffer (explicit q_off / t_off), so a scan that reads one element too far refuses a good pair.
  Positions, per side of length L and stride s of the site: 0, s - 1, s, L - 1, with L = k s + 1 so that the last stride holds one
  element; on the single-pair and multi-strip routes also 511 and 512 of the target (row 513 opens the second strip).
  What a route cannot hold (EXCLUDED) is left out.
* Non-square matrices (every non-PWM route): code 21 with a 24 x 20 and a 20 x 24 matrix, on the side where it is legal and on the
  side where it is not.
* PWM windows (batch kernels, fast and f64, and the one-workgroup route): the query side is not checked -- the bytes a query check
  would read hold 255 here --, a target code >= 4 is refused.
* Two pairs per wave: the lines in both halves, and four batches (bad, good), (good, bad), (bad, bad) and an odd batch whose last,
  partner-less item is bad; the halves come from the queue's order (queue_order()).
* check(): the comparison of a backend's answer with the oracle's, line by line.  scan_refuses(): the scans restated in Python, with
  planted faults (FAULTS), for the fake backend of the CPU test.
* The child process of tests/test_code_validation_gpu.py: python code_validation_cases.py REPORT.npz ROUTE [ROUTE ...].

Strings come back in a caller-chosen layout with GAP marker bytes between the pairs (a foreign layout: the library scatters pair by
pair and skips a failed pair), so a refused pair's region must still hold the marker.  aln_pairset_strings hands out every entry's
whole capacity, zeros where nothing was written: there a refused pair's region is zeros, as the oracle's."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import call_history as ch  # noqa: E402
import plan_cases as pc  # noqa: E402
import route_cases as rc  # noqa: E402

SITES = (
    ("pair_codes_ok in aln_fill_kernel", "generic integer batch", "64 lanes, __any"),
    ("pair_codes_ok in aln_fill_f64_kernel", "lean f64 batch and its PERPAIR build (pair sets)", "64 lanes, __any"),
    ("pair_codes_ok in aln_fill_fast_kernel", "fast, lean and cooperative builds, PWM windows", "64 lanes, with bad_shape"),
    ("inline block in aln_fill_wgpipe_kernel", "one-workgroup route", "blockDim.x threads, __syncthreads_or"),
    ("inline block in aln_fill_duo_kernel", "two pairs per wave", "lane & 31, stride 32, one __ballot split by half"),
    ("aln_validate_kernel", "in front of the single-pair route", "one wave per pair, writes desc.status"),
)
EXCLUDED = {
    "duo": "rows <= 256 (aln_plan_duo): no second strip, so no target index 511 / 512",
    "wg_*, query lines": "130 rows run R = 1, three strips, 192 threads >= rows: the target scan has one stride there; the target lines "
                         "use 601 rows (R = 2, five strips, 320 threads; the last stride is partial, not one element)",
    "pwm_*": "no query sequence; PWM never runs two pairs per wave -- aln_plan_duo: `if (!(c.fast && !c.pwm && c.semantics == "
             "ALN_CORE_GLOBAL && ...)) return;` -- nor the single-pair route -- aln_plan_routes: `single_wanted = c.fast && !c.pwm && ...`"
             " --, so the pwm argument of aln_validate_kernel is never true",
    "pwm_wg": "N = the PWM's columns; 641 rows (R = 2, six strips, 384 threads)",
}
MARK, GUARD, GAP = 0x5A, 255, 8
OK, REFUSED = 0, 3
FIELDS = ch.FIELDS
ENV = dict(ALN_TRACE_PLAN="1", ALN_BIG_TO_SINGLE="1")
SEED = 20261021
MID = 21                                 # the code of the non-square lines: 20 <= MID < 24


# ---------------------------------------------------------------- schemes
def _pwm(W):
    r = np.random.default_rng([SEED, W])
    motif = r.integers(0, 4, W)
    m = -np.ones((4, W))
    m[motif, np.arange(W)] = 2.0
    return m, motif


def scheme(name):
    """(matrix, del, ext, kernel family).  NAME, NAME:tall (24 x 20: rows > cols), NAME:wide (20 x 24)."""
    base, _, shape = name.partition(":")
    if base.startswith("PWM"):
        m, _ = _pwm(40)
        return (m, 3.0, 1.0, "fast") if base == "PWMI" else (m * 0.37 + 0.013, 1.5, 0.4, "f64")
    S, dele, ext, kind = rc.schemes()[dict(B62="INT", OFF="OFF_FAST", REAL="REAL")[base]]
    if shape == "tall":
        S = np.ascontiguousarray(S[:, :20])
    elif shape == "wide":
        S = np.ascontiguousarray(S[:20, :])
    return S, dele, ext, kind


# ---------------------------------------------------------------- routes
class Route:
    """kind: batch (aln_align_batch) | pair (aln_align_pair) | pairset (aln_pairset_run) | pwm (aln_align_batch, ALN_PWM_LOCAL).
    q_shape / t_shape: (N, M) of the lines whose byte is in the query / the target; sq / st: the site's stride there; per_batch: lines
    per batch; want: fields of the `aln route:` line of every batch; on: which list of the plan the line's pair must be in."""

    def __init__(self, name, kind, scheme, local, q_shape, sq, t_shape, st, per_batch, want, on="small", env=None, fillers=0, strips=False,
                 good=(40, 40)):
        self.name, self.kind, self.scheme, self.local = name, kind, scheme, local
        self.q_shape, self.sq, self.t_shape, self.st, self.per_batch, self.want, self.on = q_shape, sq, t_shape, st, per_batch, want, on
        self.env, self.fillers, self.strips, self.good = dict(ENV, **(env or {})), fillers, strips, good

    def pwm(self):
        return self.kind == "pwm"

    def semantics(self):
        return 4 if self.pwm() else rc.CORE_LOCAL if self.local else rc.CORE_GLOBAL

    def positions(self, side):
        """the indexes of the special byte on one side"""
        if side == "q" and self.pwm():
            return []
        (N, M), s = (self.q_shape, self.sq) if side == "q" else (self.t_shape, self.st)
        L = N if side == "q" else M
        # (a batch kernel's lines have L = k s + 1: one element in the last stride; the workgroup's s follows from the rows, so there
        # the last stride is merely partial)
        assert L > s and (L % s == 1 or (self.on == "wg" and L % s != 0)), (self.name, side, L, s)
        p = [0, s - 1, s, L - 1]
        if side == "t" and self.strips:
            assert L > 513
            p += [511, 512]
        return sorted(p)


def wg_threads(M):
    """blockDim.x of aln_fill_wgpipe_kernel for M rows: launch_wgpipe_r launches 64 * ns threads, ns = aln_uniform_strips(M, R), R by
    aln_wg_route_r."""
    R = 4 if M > 1024 else 2 if M > 512 else 1
    return 64 * ((M + 64 * R - 1) // (64 * R))


_routes = []


def routes():
    if _routes:
        return _routes
    none = dict(single=0, wg=0, duo=0, overlap=0, share="none")
    strips = dict(q_shape=(129, 577), sq=64, t_shape=(129, 577), st=64, strips=True)
    one = dict(q_shape=(129, 129), sq=64, t_shape=(129, 129), st=64)
    wg = dict(q_shape=(2 * wg_threads(130) + 1, 130), sq=wg_threads(130), t_shape=(129, 601), st=wg_threads(601), strips=True, per_batch=1, on="wg")
    big = dict(q_shape=(513, 577), sq=64, t_shape=(513, 577), st=64, strips=True, on="single")
    r = [
        Route("fast", "batch", "B62", True, per_batch=99, want=dict(none, kernels="fast"), **one),
        Route("lean", "batch", "B62", True, per_batch=99, want=dict(none, share="lean", kernels="fast"), env=dict(ALN_COOP_LEAN="1"), **strips),
        Route("coop", "batch", "B62", True, per_batch=12, want=dict(none, share="coop", kernels="fast"), **strips),
        Route("duo", "batch", "B62", False, (65, 65), 32, (65, 65), 32, 99, dict(none, duo=1, kernels="fast"), fillers=12 * rc.CUS + 8, good=(30, 30)),
        Route("int", "batch", "OFF", True, per_batch=99, want=dict(none, kernels="int"), **one),
        Route("f64", "batch", "REAL", True, per_batch=99, want=dict(none, kernels="f64"), **one),
        Route("pairset", "pairset", "REAL", True, per_batch=99, want=dict(none, kernels="f64"), **one),
        Route("wg_int", "batch", "OFF", True, want=dict(none, wg=1, small=2, kernels="int"), **wg),
        Route("wg_real", "batch", "REAL", True, want=dict(none, wg=1, small=2, kernels="f64"), **wg),
        Route("single_pair", "pair", "B62", True, per_batch=1, want=dict(none, single=1, small=0, kernels="fast"), **big),
        Route("single_batch", "batch", "B62", True, per_batch=7, want=dict(wg=0, duo=0, overlap=0, share="none", kernels="fast"), **big),
        Route("pwm_fast", "pwm", "PWMI", True, None, 0, (40, 129), 64, 99, dict(none, kernels="fast")),
        Route("pwm_f64", "pwm", "PWMR", True, None, 0, (40, 129), 64, 99, dict(none, kernels="f64")),
        Route("pwm_wg", "pwm", "PWMR", True, None, 0, (40, 641), wg_threads(641), 1, dict(none, wg=1, small=2, kernels="f64"), on="wg"),
    ]
    assert wg_threads(130) == 192 and wg_threads(601) == 320 and wg_threads(641) == 384
    _routes.extend(r)
    return _routes


def route(name):
    return next(r for r in routes() if r.name == name)


# ---------------------------------------------------------------- sequences
def _related(rng, n, m, A):
    q = rng.integers(0, A, n).astype(np.uint8)
    t = rng.integers(0, A, m).astype(np.uint8)
    L = (3 * min(n, m)) // 4
    a, b = int(rng.integers(0, n - L + 1)), int(rng.integers(0, m - L + 1))
    run = q[a:a + L].copy()
    mut = rng.random(L) < 0.08
    run[mut] = rng.integers(0, A, int(mut.sum()))
    t[b:b + L] = run
    return q, t


def _window(rng, m, motif):
    """a PWM window of m residues that holds the motif (or its first m positions), a tenth of it mutated"""
    W = len(motif)
    t = rng.integers(0, 4, m).astype(np.uint8)
    L = min(m, W)
    a = int(rng.integers(0, m - L + 1))
    t[a:a + L] = np.where(rng.random(L) < 0.1, rng.integers(0, 4, L), motif[:L])
    return np.zeros(0, np.uint8), t


class Line:
    def __init__(self, name, side, pos, value, bad):
        self.name, self.side, self.pos, self.value, self.bad = name, side, pos, value, bad
        self.half = None                 # two pairs per wave: the half of the wave this line must run in


class Batch:
    """pairs: [(q, t)]; lines: {pair number: Line}; every other pair is a good neighbour.  The packed buffer holds a guard byte before
    and after every sequence."""

    def __init__(self, name, rt, scheme_name, pairs, lines):
        self.name, self.route, self.scheme_name, self.pairs, self.lines = name, rt, scheme_name, pairs, lines
        chunks, q_off, t_off, pos = [np.full(1, GUARD, np.uint8)], [], [], 1
        for q, t in pairs:
            for s, off in ((q, q_off), (t, t_off)):
                off.append(pos)
                if len(s):
                    chunks += [s, np.full(1, GUARD, np.uint8)]
                    pos += len(s) + 1
        self.seqs = np.concatenate(chunks)
        self.q_off, self.t_off = np.array(q_off, np.uint64), np.array(t_off, np.uint64)
        self.q_len = np.array([len(q) for q, _ in pairs], np.uint64)
        self.t_len = np.array([len(t) for _, t in pairs], np.uint64)

    def __len__(self):
        return len(self.pairs)

    def scheme(self):
        return scheme(self.scheme_name)

    def dims(self):
        S = self.scheme()[0]
        return S.shape                   # rows (target codes), cols (query codes; PWM: positions)

    def columns(self):
        """N per pair as the kernels see it"""
        return np.full(len(self), self.dims()[1], np.int64) if self.route.pwm() else self.q_len.astype(np.int64)

    def caps(self):
        return self.columns() + self.t_len.astype(np.int64) + 2

    def tb_layout(self):
        """(offsets, total): every pair's region (2 cap bytes; PWM: 5 cap, 4-aligned), then GAP bytes that nobody may write.  A pair
        set's strings come back for the listed entries in the documented cumulative layout (no gaps)."""
        cap = self.caps()
        size = ((5 * cap + 3) & ~3) if self.route.pwm() else 2 * cap
        gap = 0 if self.route.kind == "pairset" else GAP
        off = np.concatenate([[0], np.cumsum(size + gap)[:-1]]).astype(np.uint64)
        return off, size, int((size + gap).sum())

    def guarded(self):
        """every sequence has a guard byte directly before and directly after it"""
        s = self.seqs
        for off, ln in list(zip(self.q_off, self.q_len)) + list(zip(self.t_off, self.t_len)):
            if ln and not (s[int(off) - 1] == GUARD and s[int(off + ln)] == GUARD):
                return False
        return True


def _put(pair, side, pos, value):
    q, t = pair[0].copy(), pair[1].copy()
    (q if side == "q" else t)[pos] = value
    return q, t


def _interleave(rng, rt, A, specials, motif=None):
    """good, special, good, special, ..., good"""
    def good():
        return _window(rng, rt.good[1], motif) if rt.pwm() else _related(rng, rt.good[0], rt.good[1], A)
    if rt.kind == "pair":                            # aln_align_pair takes one pair
        (ln, pair), = specials
        return [pair], {0: ln}
    pairs, lines = [good()], {}
    if rt.pwm():
        pairs[0] = _window(rng, 5, motif)            # the lowest offset: the bytes a query check would read end in its guard byte
    for ln, pair in specials:
        lines[len(pairs)] = ln
        pairs += [pair, good()]
    return pairs, lines


def queue_order(N, M):
    """The batch kernel's queue of a chunk whose pairs all take it: by falling aln_pair_cost, equal costs by rising pair number
    (aln_plan_order); tests/test_code_validation_cpu.py holds it against the header's."""
    cost = [pc.pair_cost(int(n), int(m)) for n, m in zip(N, M)]
    return sorted(range(len(cost)), key=lambda i: (-cost[i], i))


def halves(b):
    """pair number -> (queue item, half) of a two-pairs-per-wave batch: item i takes queue positions 2 i and 2 i + 1"""
    return {i: (qpos // 2, qpos & 1) for qpos, i in enumerate(queue_order(b.columns(), b.t_len))}


_batches = {}


def batches(rt):
    """The batches of a route, built once per process from a seed of the route's own."""
    if rt.name in _batches:
        return _batches[rt.name]
    rng = np.random.default_rng([SEED, routes().index(rt)])
    out = []
    rows, cols = scheme(rt.scheme)[0].shape
    motif = _pwm(cols)[1] if rt.pwm() else None
    A = 4 if rt.pwm() else 20
    # 1. the positions: per side, index and value a bad line and its twin
    specials = []
    for side in ("q", "t"):
        dim = cols if side == "q" else rows
        for pos in rt.positions(side):
            for value in (dim, 255):
                shape = rt.q_shape if side == "q" else rt.t_shape
                base = _window(rng, shape[1], motif) if rt.pwm() else _related(rng, shape[0], shape[1], A)
                tag = "%s/%s%d/%s" % (rt.name, side, pos, "edge" if value == dim else "255")
                duo = [(Line(tag, side, pos, value, True), _put(base, side, pos, value)),
                       (Line(tag + "/twin", side, pos, dim - 1, False), _put(base, side, pos, dim - 1))]
                specials += duo[::-1] if rt.fillers and (len(specials) // 2) % 2 else duo
    if rt.fillers:
        # two pairs per wave: the lines cost the most and head the queue in their own order, a bad line and its twin in one wave
        pairs, lines = _interleave(rng, rt, A, specials)
        pairs += [_related(rng, rt.good[0], rt.good[1], A) for _ in range(rt.fillers)]
        b = Batch(rt.name + "/positions", rt, rt.scheme, pairs, lines)
        for i, (item, half) in halves(b).items():
            if i in lines:
                lines[i].half = half
        out.append(b)
    else:
        for k in range(0, len(specials), rt.per_batch):
            pairs, lines = _interleave(rng, rt, A, specials[k:k + rt.per_batch], motif)
            out.append(Batch("%s/positions%d" % (rt.name, k // rt.per_batch), rt, rt.scheme, pairs, lines))
    # 2. non-square matrices: MID on the side where it is legal and on the side where it is not
    if not rt.pwm():
        for shape_name, legal in (("tall", "t"), ("wide", "q")):
            specials = []
            for side in ("q", "t"):
                N, M = rt.q_shape if side == "q" else rt.t_shape
                base = _related(rng, N, M, A)
                pos = (N if side == "q" else M) // 2
                tag = "%s/%s/%s%d/%s" % (rt.name, shape_name, side, pos, "legal" if side == legal else "illegal")
                specials.append((Line(tag, side, pos, MID, side != legal), _put(base, side, pos, MID)))
            for k in range(0, 2, rt.per_batch):
                pairs, lines = _interleave(rng, rt, A, specials[k:k + rt.per_batch])
                pairs += [_related(rng, rt.good[0], rt.good[1], A) for _ in range(rt.fillers)]
                out.append(Batch("%s/%s%d" % (rt.name, shape_name, k), rt, rt.scheme + ":" + shape_name, pairs, lines))
    # 3. two pairs per wave: the two halves against each other, and a partner-less last item
    if rt.fillers:
        N, M = rt.t_shape
        for name, flags in (("bad_good", (1, 0)), ("good_bad", (0, 1)), ("bad_bad", (1, 1, 0, 0)), ("odd", (0, 0))):
            pairs, lines = [], {}
            for j, bad in enumerate(flags):
                base = _related(rng, N, M, A)
                side = "qt"[j % 2]
                pos = (N - 1) if j % 2 == 0 else 0
                value = (cols if side == "q" else rows) - (0 if bad else 1)
                ln = Line("%s/%s/%d" % (rt.name, name, j), side, pos, value, bool(bad))
                ln.half = j & 1
                lines[len(pairs)] = ln
                pairs.append(_put(base, side, pos, value))
            pairs += [_related(rng, rt.good[0], rt.good[1], A) for _ in range(rt.fillers + (len(flags) & 1))]
            if name == "odd":                        # the cheapest pair: the queue's last position, alone in its wave
                assert len(pairs) % 2 == 0
                ln = Line("%s/odd/last" % rt.name, "t", 23, rows, True)
                ln.half = 0
                lines[len(pairs)] = ln
                pairs.append(_put(_related(rng, 24, 24, A), "t", 23, rows))
            out.append(Batch("%s/%s" % (rt.name, name), rt, rt.scheme, pairs, lines))
    assert len({b.name for b in out}) == len(out)
    _batches[rt.name] = out
    return out


def pair_matrices(b):
    """aln_pairset_run: a matrix per pair -- the scheme's, pair k's lowered by k * 2^-20 in entry (0, 0) so that no two are the same"""
    S = b.scheme()[0]
    m = np.repeat(S[None], len(b), axis=0).copy()
    m[:, 0, 0] -= np.arange(len(b)) * 2.0 ** -20
    return m


# ---------------------------------------------------------------- the plan
def planned(b):
    """route_cases.plan() of a batch under its route's knobs"""
    S, dele, ext, kind = b.scheme()
    return rc.plan(b.columns(), b.t_len.astype(np.int64), kind, b.route.local, dele, ext, True, b.route.env)


def route_problems(b, line):
    """What is wrong with a batch's `aln route:` line (a dict of route_cases.parse_routes), or []"""
    p, out = planned(b), []
    want = dict(rc.line_of(p))
    if line != want:
        out.append("%s: route line %s, planned %s" % (b.name, line, want))
    for k, v in b.route.want.items():
        if line.get(k) != v:
            out.append("%s: route line has %s %s, the route wants %s" % (b.name, k, line.get(k), v))
    for i, ln in b.lines.items():
        on = "single" if p["single_mask"][i] else "wg" if p["wg_mask"][i] else "small"
        if on != b.route.on:
            out.append("%s: planned onto %s, not %s" % (ln.name, on, b.route.on))
    return out


def plan_facts(b):
    """the call's facts as plan_call (aln_host.hip) hands them to the plan, in the order of plan_cases.FACTS"""
    S, dele, ext, kind = b.scheme()
    rt = b.route
    return dict(pwm=rt.pwm(), fast=kind == "fast", is_int=kind != "f64", want_h=0, want_tb=1, store_dirs=1,
                semantics=rc.CORE_LOCAL if rt.pwm() else rt.semantics(), rows=S.shape[0], cols=S.shape[1], hazard=int(rt.local and dele != ext),
                force_serial=0, pair_matrices=rt.kind == "pairset")


def plan_case(b):
    spec = "+".join("%dx%d" % (n, m) for n, m in zip(b.columns(), b.t_len))
    env = {k: v for k, v in b.route.env.items() if k != "ALN_TRACE_PLAN"}
    return pc.case(b.name, spec, "PWM" if b.route.pwm() else "INT", local=b.route.local, env=env)


# ---------------------------------------------------------------- the oracle's answers
def expected(orc, b):
    """status and every summary field per pair, and the strings in the batch's own layout (tb_layout) on a marker-filled buffer:
    what a backend must hand back, byte for byte where `known` is set (capacity beyond aln_len is unspecified)."""
    S, dele, ext, _ = b.scheme()
    n = len(b)
    off, size, total = b.tb_layout()
    fill = 0 if b.route.kind == "pairset" else MARK
    tb = np.full(total, fill, np.uint8)
    known = np.ones(total, bool)
    want = {f: np.zeros(n, ch.ORC_DTYPE[f]) for f in FIELDS}
    cap = b.caps()
    if b.route.pwm():
        for i, (_, t) in enumerate(b.pairs):
            r = orc.align_pwm(t, dele, ext, S)
            rec = dict(status=r["status"], score=r["score"], f=r["f"], end_y=r["end"][0], end_x=r["end"][1], start_y=r["start"][0],
                       start_x=r["start"][1], aln_len=len(r["numbered"]))
            for f in FIELDS:
                want[f][i] = rec[f]
            if r["status"] == OK:
                o, L, c = int(off[i]), len(r["numbered"]), int(cap[i])
                known[o:o + int(size[i])] = False
                tb[o:o + 4 * L] = r["numbered"].astype("<u4").view(np.uint8)
                tb[o + 4 * c:o + 4 * c + L] = r["qal"]
                known[o:o + 4 * L] = True
                known[o + 4 * c:o + 4 * c + L] = True
    else:
        mats = pair_matrices(b) if b.route.kind == "pairset" else None
        for i, (q, t) in enumerate(b.pairs):
            r = orc.align(b.route.semantics(), q, t, dele, ext, S if mats is None else mats[i])
            rec = dict(status=r["status"], score=r["score"], f=r["f"], end_y=r["end"][0], end_x=r["end"][1], start_y=r["start"][0],
                       start_x=r["start"][1], aln_len=len(r["qa"]))
            for f in FIELDS:
                want[f][i] = rec[f]
            if r["status"] == OK:
                o, L, c = int(off[i]), len(r["qa"]), int(cap[i])
                if b.route.kind != "pairset":
                    known[o:o + 2 * c] = False
                tb[o:o + L] = r["qa"]
                tb[o + c:o + c + L] = r["ta"]
                known[o:o + L] = True
                known[o + c:o + c + L] = True
    want["tb"], want["known"] = tb, known
    return want


def check(b, got, want):
    """[(line name | pair, what differs)]: a backend's answer (results: RESULT_DTYPE records; tb: the marker-filled buffer after the
    call) against expected().  Nothing is tolerated."""
    out = []
    res, off, size = got["results"], *b.tb_layout()[:2]

    def name(i):
        return b.lines[i].name if i in b.lines else "%s/good%d" % (b.name, i)
    for i in range(len(b)):
        bad = [f for f in FIELDS if res[f][i] != want[f][i] and not (res[f][i] != res[f][i] and want[f][i] != want[f][i])]
        if want["status"][i] != OK and (res["passes"][i] != 0 or res["flags"][i] != 0):
            bad.append("passes/flags of a refused pair")
        o, s = int(off[i]), int(size[i])
        k = want["known"][o:o + s]
        if not np.array_equal(got["tb"][o:o + s][k], want["tb"][o:o + s][k]):
            bad.append("strings" if want["status"][i] == OK else "the string region of a refused pair was written")
        if bad:
            out.append((name(i), "%s: got status %d f %r, want status %d f %r" % (", ".join(bad), res["status"][i], float(res["f"][i]),
                                                                                   want["status"][i], float(want["f"][i]))))
    gaps = np.ones(len(want["tb"]), bool)
    for o, s in zip(off, size):
        gaps[int(o):int(o + s)] = False
    if not np.array_equal(got["tb"][gaps], want["tb"][gaps]):
        out.append((b.name, "bytes between the pairs' string regions were written"))
    return out


def flag_problems(b, got):
    """the flags word of every pair that succeeded names the planned kernels (route_cases.want_flags)"""
    p = planned(b)
    mask, val = rc.want_flags(p, p["kernels"])
    ok = got["results"]["status"] == OK
    wrong = np.flatnonzero(ok & ((got["results"]["flags"] & mask) != val))
    return ["%s: pair %d has flags %#x, planned %#x" % (b.name, i, got["results"]["flags"][i], val[i]) for i in wrong]


# ---------------------------------------------------------------- the scans, restated (the fake backend of the CPU test)
FAULTS = ("gt_for_ge", "stops_at_last_whole_stride", "starts_at_index_1", "both_sides_against_cols", "query_checked_under_pwm",
          "duo_verdict_from_whole_ballot", "reads_one_byte_past_the_end")


def _scan_hits(seqs, off, L, s, dim, fault):
    """a strided scan of seqs[off .. off + L) by s lanes: does any lane see a code the matrix does not score?"""
    end = L
    if fault == "stops_at_last_whole_stride":
        end = (L // s) * s
    elif fault == "reads_one_byte_past_the_end":
        end = L + 1
    first = 1 if fault == "starts_at_index_1" else 0
    for lane in range(s):
        i = lane + first
        while i < end:
            v = int(seqs[off + i])
            if (v > dim) if fault == "gt_for_ge" else (v >= dim):
                return True
            i += s
    return False


def scan_refuses(b, fault=None):
    """Per pair: does the route's site refuse it?  The scans of aln_kernels.hip restated on the host's buffer, one planted fault at
    most.  (PWM: the query a check would read is the first N bytes of the residues the call uploads.)"""
    rows, cols = b.dims()
    rt = b.route
    lo = int(b.t_off.min())
    N = b.columns()
    bad = np.zeros(len(b), bool)
    for i in range(len(b)):
        M = int(b.t_len[i])
        if rt.fillers:
            sq = st = 32
        elif rt.on == "wg" and planned(b)["wg_mask"][i]:
            sq = st = wg_threads(M)
        else:
            sq = st = 64
        t_dim = cols if fault == "both_sides_against_cols" else rows
        hit = _scan_hits(b.seqs, int(b.t_off[i]), M, st, t_dim, fault)
        if not rt.pwm():
            hit = hit or _scan_hits(b.seqs, int(b.q_off[i]), int(N[i]), sq, cols, fault)
        elif fault == "query_checked_under_pwm":
            hit = hit or _scan_hits(b.seqs, lo, int(N[i]), sq, cols, None)
        bad[i] = hit
    if rt.fillers and fault == "duo_verdict_from_whole_ballot":
        order = queue_order(N, b.t_len)
        for k in range(0, len(order) - 1, 2):
            bad[order[k]] = bad[order[k + 1]] = bad[order[k]] or bad[order[k + 1]]
    return bad


def fake_answer(b, want, fault=None):
    """What a library whose scan has the given fault would hand back: the oracle's answer where its scan agrees with the truth, a
    refusal where it refuses a good pair, and a made-up success (the fill read beyond the matrix) where it lets a bad pair through."""
    from aligner_amd.batch import RESULT_DTYPE
    refuse = scan_refuses(b, fault)
    res = np.zeros(len(b), RESULT_DTYPE)
    tb = want["tb"].copy()
    off, size, _ = b.tb_layout()
    for i in range(len(b)):
        truly_bad = want["status"][i] != OK
        if refuse[i] == truly_bad:
            for f in FIELDS:
                res[f][i] = want[f][i]
        elif refuse[i]:
            res["status"][i] = REFUSED
            tb[int(off[i]):int(off[i] + size[i])] = 0 if b.route.kind == "pairset" else MARK
        else:
            res["status"][i], res["f"][i], res["score"][i], res["aln_len"][i] = OK, 1.0, 1.0, 1
    return dict(results=res, tb=tb)


# ---------------------------------------------------------------- the child process of tests/test_code_validation_gpu.py
def _params(b, outputs):
    from aligner_amd import runtime
    S, dele, ext, _ = b.scheme()
    return runtime.make_params(b.route.semantics(), dele, ext, S, outputs=outputs)


def run_gpu(b):
    """One batch through the C ABI on marker-filled buffers: dict(results, tb, call) -- call: the call's own return value."""
    from aligner_amd import _ffi, runtime
    from aligner_amd.batch import RESULT_DTYPE
    lib, n = _ffi.load(), len(b)
    off, size, total = b.tb_layout()
    res = np.frombuffer(bytes([MARK]) * (48 * n), dtype=RESULT_DTYPE).copy()
    tb = np.full(total, MARK, np.uint8)
    outs = _ffi.OUT_SCORE | _ffi.OUT_TRACEBACK
    kind = b.route.kind
    if kind in ("batch", "pwm"):
        p, keep = _params(b, outs)
        q_len = b.columns().astype(np.uint64)
        q_off = np.zeros(n, np.uint64) if kind == "pwm" else b.q_off
        st = lib.aln_align_batch(runtime.context(), C.byref(p), b.seqs.ctypes.data, q_off.ctypes.data, q_len.ctypes.data, b.t_off.ctypes.data,
                                 b.t_len.ctypes.data, n, res.ctypes.data, tb.ctypes.data, off.ctypes.data)
    elif kind == "pair":
        assert n == 1
        p, keep = _params(b, 0)
        r = _ffi.PairResult()
        cap = int(b.caps()[0])
        q, t = int(b.q_off[0]), int(b.t_off[0])
        st = lib.aln_align_pair(runtime.context(), C.byref(p), b.seqs.ctypes.data + q, int(b.q_len[0]), b.seqs.ctypes.data + t, int(b.t_len[0]),
                                C.byref(r), tb.ctypes.data, tb.ctypes.data + cap, None, None)
        res = np.frombuffer(bytes(r), dtype=RESULT_DTYPE).copy()
        st = 0 if st == res["status"][0] else -1000 - st      # the call returns the pair's status
    else:
        from aligner_amd.batch import PairBatch
        from aligner_amd.pairset import PairSet
        S, dele, ext, _ = b.scheme()
        with PairSet(PairBatch(b.seqs, b.q_off, b.q_len, b.t_off, b.t_len)) as ps:
            act = np.arange(n, dtype=np.uint32)
            m = pair_matrices(b)
            p = _ffi.Params(b.route.semantics(), 0, float(dele), float(ext), None, m.shape[1], m.shape[2], m.shape[2], 0, 98, 0, 0, 0, 0)
            run = np.zeros(n, RESULT_DTYPE)
            st = lib.aln_pairset_run(ps.handle, C.byref(p), m.ctypes.data, act.ctypes.data, n, run.ctypes.data)
            if st == OK:                 # (a failed pair is a status in its summary, not the call's)
                st = lib.aln_pairset_strings(ps.handle, act.ctypes.data, n, res.ctypes.data, tb.ctypes.data, off.ctypes.data)
                if st == OK and run.tobytes() != res.tobytes():
                    st = -2000
    return dict(results=res, tb=tb, call=np.asarray(st))


def main(argv):
    from aligner_amd import runtime
    report, names = argv[0], argv[1:]
    out = {}
    runtime.context()                    # (aln_create warms up with a pair of its own: its route line comes before the first marker)
    for name in names:
        for b in batches(route(name)):
            rc.mark(b.name)
            got = run_gpu(b)
            for k, v in got.items():
                out[b.name + "|" + k] = v
    np.savez(report, **out)


if __name__ == "__main__":
    main(sys.argv[1:])
