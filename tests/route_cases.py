"""Helpers of the set-route tests (tests/test_set_routes_*.py).  Not a test module (no test_ prefix).

* One seeded pool of 102 sequences over the 24 x 24 BLOSUM62 alphabet: 92 short ones (20 .. 120 residues, mutated pieces of one
  700-residue ancestor, each holding residue 0) and ten long ones (130 .. 2600: the ancestor repeated, 10 % substitutions, three
  block indels of 5 .. 40; a second 600 ends in code 24, which no 24 x 24 matrix scores).  A block of a sequence set is two RANGES
  of sequence numbers, so the resident set lists the 92 shorts once and then, block by block, the members of every other block's
  ranges again (LAYOUT: 118 entries over the 102 sequences).
* A table of blocks on that set (blocks()), one per route of the batch plan (aln_plan_rules.h), with the scheme that selects it.
* plan(): the routing of chunk_plan restated as arithmetic on lengths and counts, with the knobs the tests set -- what an
  `aln route:` line (ALN_TRACE_PLAN) must say for a list of pairs.  The comments name the steps of aln_plan_chunk
  (aligner_amd/csrc/aln_plan_rules.h); tests/test_plan_rules_cpu.py checks plan() against those steps on every block.
* The child processes of tests/test_set_routes_gpu.py: python route_cases.py MODE expected.npz report.json [block].
"""
import hashlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import call_history as ch  # noqa: E402
from scheme_limits import FAST_SMAX  # noqa: E402

CORE_GLOBAL, CORE_LOCAL = 0, 1          # _ffi.CORE_GLOBAL, _ffi.CORE_LOCAL
OK, ERR_CODE_OUT_OF_RANGE = 0, 3
FLAG_INTEGER, FLAG_SINGLE, FLAG_WORKGROUP, FLAG_FAST = 1, 2, 4, 8
CUS = ch.CUS
STRIP_ROWS = ch.STRIP_ROWS
SEED = 20261019
N_SHORT = 92
LONG_LENGTHS = (130, 300, 520, 600, 640, 700, 900, 1100, 2600)
BAD = "B600"
KMER = (2, 24)                           # the prefilter's words: with both thresholds 0 every pair of a block is a candidate
CHILD_ENV = dict(ALN_TRACE_PLAN="1", ALN_TB_OVERLAP_ANY="1", ALN_BIG_TO_SINGLE="1")
SUMMARY = ch.FIELDS


# ---------------------------------------------------------------- the sequences
def _long(rng, anc, L):
    base = np.tile(anc, (L + 400) // len(anc) + 2)[:L + 300].copy()
    for _ in range(3):
        p, w = int(rng.integers(50, len(base) - 50)), int(rng.integers(5, 41))
        base = np.delete(base, slice(p, p + w)) if rng.random() < 0.5 else np.insert(base, p, rng.integers(0, 20, w).astype(np.uint8))
    s = base[:L].copy()
    mut = rng.random(L) < 0.10
    s[mut] = rng.integers(0, 20, int(mut.sum()))
    return s.astype(np.uint8)


_pool = {}


def pool():
    """name -> codes: s0 .. s91 (s0 has 30 residues, s91 has 40), L130 .. L2600, B600."""
    if _pool:
        return _pool
    rng = np.random.default_rng(SEED)
    anc = rng.integers(0, 20, 700).astype(np.uint8)
    lengths = [30] + [int(v) for v in rng.integers(20, 121, N_SHORT - 2)] + [40]
    for i, L in enumerate(lengths):
        a = int(rng.integers(0, 200))
        s = anc[a:a + L].copy()
        mut = rng.random(L) < rng.uniform(0.05, 0.5)
        s[mut] = rng.integers(0, 20, int(mut.sum()))
        s[int(rng.integers(0, L))] = 0
        _pool["s%d" % i] = s
    for L in LONG_LENGTHS:
        _pool["L%d" % L] = _long(rng, anc, L)
    bad = _long(rng, anc, 600)
    bad[-1] = 24
    _pool[BAD] = bad
    return _pool


SHORTS = ["s%d" % i for i in range(N_SHORT)]
LAYOUT = SHORTS + [
    "L600", "L640",                                                  # single_alone
    "L520", BAD, "s91", "L640", "L2600", "s0",                       # single_mixed: queries, targets
    "L130", "L520", "L600", "L640", "L700", "L900", "L1100",         # coop
    "L300", "L600", "L130", "L640",                                  # wg_real: queries, targets
    "L300", "L130", "s91", "L1100",                                  # wg_mixed: query, targets
    "L300", "L520", "L130",                                          # wg_int: queries, target
]


def set_codes():
    p = pool()
    return [p[name] for name in LAYOUT]


def set_lengths():
    return np.array([len(c) for c in set_codes()], dtype=np.int64)


# ---------------------------------------------------------------- the schemes
def schemes():
    from aligner_amd.matrices import get_blosum62
    b62 = np.asarray(get_blosum62(), dtype=np.float64)
    off = b62.copy()
    i = int(np.argmax(np.diag(off)))
    off[i, i] = FAST_SMAX + 1            # one entry beyond the int8 profile of the fast kernels (aln_scheme_rules.h)
    return dict(INT=(b62, 11.0, 2.0, "fast"), INT44=(b62, 4.0, 4.0, "fast"), REAL=(b62 * 0.37 + 0.013, 11.3, 2.1, "f64"),
                OFF_FAST=(off, 11.0, 2.0, "int"))


# ---------------------------------------------------------------- the blocks
class Block:
    """q0, qn, t0, tn: the ranges in LAYOUT; upper: the pairs i < j of the square q0 .. q0 + qn - 1.  want: what the `aln route:`
    line of the held pass over every pair that succeeds must show (the table of the tests' docstrings)."""

    def __init__(self, name, q0, qn, t0, tn, upper, scheme, semantics, want, names=None):
        self.name, self.q0, self.qn, self.t0, self.tn, self.upper = name, q0, qn, t0, tn, upper
        self.scheme, self.semantics, self.want = scheme, semantics, want
        self.names = names               # (query names, target names): what the ranges must hold

    def tuple(self):
        return (self.q0, self.qn, self.t0, self.tn, 1 if self.upper else 0)

    def pairs(self):
        """(q, t): sequence numbers of every pair, in the block's order (aln_seqset_rules.h)."""
        if self.upper:
            q, t = np.triu_indices(self.qn, 1)
            return q + self.q0, t + self.q0
        return np.repeat(np.arange(self.q0, self.q0 + self.qn), self.tn), np.tile(np.arange(self.t0, self.t0 + self.tn), self.qn)

    def local(self):
        return self.semantics == CORE_LOCAL


def _at(names, after=N_SHORT):
    for i in range(after, len(LAYOUT) - len(names) + 1):
        if LAYOUT[i:i + len(names)] == list(names):
            return i
    raise AssertionError(names)


def _rect(name, qn, tn, scheme, want, semantics=CORE_LOCAL):
    q0 = _at(list(qn) + list(tn))
    return Block(name, q0, len(qn), q0 + len(qn), len(tn), False, scheme, semantics, want, (list(qn), list(tn)))


_blocks = []


def blocks():
    """The eight blocks of the schedule, then single_mixed again under core global."""
    if _blocks:
        return _blocks
    mixed = (["L520", BAD, "s91"], ["L640", "L2600", "s0"])
    coop = ["L130", "L520", "L600", "L640", "L700", "L900", "L1100"]
    b = [
        Block("duo", 0, 60, 32, 60, False, "INT44", CORE_GLOBAL, dict(small=3600, single=0, wg=0, duo=1, overlap=0, share="none", kernels="fast")),
        Block("overlap", 0, N_SHORT, 0, N_SHORT, True, "INT", CORE_LOCAL, dict(small=4186, single=0, wg=0, duo=0, overlap=1, share="none", kernels="fast")),
        _rect("single_alone", ["L600"], ["L640"], "INT", dict(small=0, single=1, wg=0, duo=0, overlap=0, share="none", kernels="fast")),
        _rect("single_mixed", *mixed, "INT", dict(small=4, single=2, wg=0, duo=0, overlap=0, kernels="fast")),
        Block("coop", _at(coop), 7, _at(coop), 7, True, "INT", CORE_LOCAL, dict(small=21, single=0, wg=0, duo=0, overlap=0, share="coop", kernels="fast"),
              (coop, coop)),
        _rect("wg_real", ["L300", "L600"], ["L130", "L640"], "REAL", dict(small=0, single=0, wg=4, duo=0, overlap=0, share="none", kernels="f64")),
        _rect("wg_mixed", ["L300"], ["L130", "s91", "L1100"], "REAL", dict(small=1, single=0, wg=2, duo=0, overlap=0, share="none", kernels="f64")),
        _rect("wg_int", ["L300", "L520"], ["L130"], "OFF_FAST", dict(small=0, single=0, wg=2, duo=0, overlap=0, share="none", kernels="int")),
        _rect("single_mixed_global", *mixed, "INT", dict(small=4, single=2, wg=0, duo=0, overlap=0, kernels="fast"), CORE_GLOBAL),
    ]
    _blocks.extend(b)
    return _blocks


SCHEDULE_BLOCKS = 8


def block(name):
    return next(b for b in blocks() if b.name == name)


# ---------------------------------------------------------------- chunk_plan's routing, restated
def strips(m):
    return (np.asarray(m, dtype=np.int64) + STRIP_ROWS - 1) // STRIP_ROWS


def plan(N, M, kind, local, dele, ext, traceback, env=(), alone=True):
    """What chunk_plan decides for one chunk of pairs with N columns (query) and M rows (target), every pair valid: a dict with the
    fields of the `aln route:` line, and the masks `single_mask` / `wg_mask`.  kind: the call's kernel family (fast | int | f64);
    traceback: a held pass (directions and strings); alone: a single-chunk call; env: the knobs that are set."""
    env = dict(env)
    N, M = np.asarray(N, dtype=np.int64), np.asarray(M, dtype=np.int64)
    n, pc, fast = len(N), N * M, kind == "fast"
    assert n and (N > 0).all() and (M > 0).all() and max(N.max(), M.max()) <= 8192
    # a large pair, or a sizeable one in a chunk of at most 16 (aln_big_pair)
    big = (N >= 64) & (M >= 128) & ((pc >= 1 << 24) | ((n <= 16) & (pc >= 1 << 18)))
    coop_on = fast and "ALN_NO_COOP" not in env                                            # aln_coop_on
    big_to_single = True
    if coop_on and big.any():                                                              # the time rule, aln_big_to_single
        lat = (N + 63.0 + 170.0 * (strips(M) - 1.0)) * 0.55e-6
        waves = CUS * 12.0

        def t_batch(cells, st, la):
            return 0.0 if cells <= 0 else max(cells / 2.6e12, la, cells / (min(st, waves) * 0.85e9))

        t_single = float((pc[big] / 60e9 + 0.2e-3).sum())
        sm = ~big
        rest = t_batch(float(pc[sm].sum()), float(strips(M[sm]).sum()), float(lat[sm].max()) if sm.any() else 0.0)
        big_to_single = t_single + rest <= t_batch(float(pc.sum()), float(strips(M).sum()), float(lat.max()))
        if "ALN_BIG_TO_SINGLE" in env:
            big_to_single = int(env["ALN_BIG_TO_SINGLE"]) != 0
    single = big & fast & (big_to_single | (strips(M) > 64))                               # aln_plan_routes (N <= 8192: the LDS bound of aln_single_route_r is far)
    # generic kernels, a chunk of at most four pairs: one workgroup per pair (aln_wg_route_r; aln_wg_lds_bytes is far below 64 KiB here)
    wg = ~single & (not fast) & ("ALN_NO_WGPIPE" not in env) & (n <= 4) & (pc >= 1 << 14) & (N >= 16) & (N <= 8192) & (M >= 65) & (M <= 2048)
    small = ~single & ~wg
    n_small = int(small.sum())
    r = dict(pairs=n, small=n_small, single=int(single.sum()), wg=int(wg.sum()), kernels=kind, single_mask=single, wg_mask=wg)
    # walk waves beside the fill (aln_plan_grid): a held pass of at least 4096 pairs that fill the chip, integer fast kernels
    wg_needed = (n_small + 3) // 4
    r["overlap"] = int(alone and env.get("ALN_TB_OVERLAP") != "0" and fast and traceback and n_small >= 4096 and wg_needed >= 3 * CUS and
                       (int(pc.sum()) >= 2000000000 or "ALN_TB_OVERLAP_ANY" in env))
    # something to share (aln_plan_share): several strips, or a re-fill of a core-local pair with del != ext that is large enough to matter
    multi = (M[small] > STRIP_ROWS) | (bool(local and dele != ext) & (M[small] > 64) & (pc[small] >= 1 << 18))
    coop = bool(coop_on and n_small and multi.any())                                       # aln_plan_share (one chunk, or at most four)
    # the lean build needs 16 pairs per kernel wave (aln_plan_rules.h); the grid is at least one workgroup of four.  ALN_COOP_LEAN
    # decides by itself (aln_coop_lean_plan's setting: 0 never lean, > 0 always lean)
    lean = False
    if coop and "ALN_COOP_LEAN" in env:
        lean = int(env["ALN_COOP_LEAN"]) > 0
        coop = not lean
    else:
        assert not (coop and n_small >= 64), "a block that could run the lean build: restate aln_coop_lean_plan"
    r["share"] = "coop" if coop else "lean" if lean else "none"
    coop = coop or lean                                                                    # (aln_plan_duo: neither build)
    # two pairs per wave (aln_plan_duo): core global, nothing shared, no walk waves, more pairs than 12 per CU, short pairs, LDS (24 x 24)
    duo = fast and not local and not coop and not r["overlap"] and "ALN_NO_DUO" not in env and n_small > CUS * 12
    if duo:
        rows, cols = int(M[small].max()), int(N[small].max())
        rmax = (rows + 31) // 32
        rp = 8 if rmax > 4 else 4 if rmax > 2 else max(rmax, 1)
        lds = ((24 * 24 * 4 + 15) & ~15) + 4 * (24 * 64 * rp + 4 * ((cols + 136 + 7) & ~7))
        duo = rows <= 256 and cols <= 1024 and lds <= 52 * 1024
    r["duo"] = int(bool(duo))
    return r


ROUTE = re.compile(r"aln route: pairs (\d+) small (\d+) single (\d+) wg (\d+) duo ([01]) overlap ([01]) share (\w+) kernels (\w+)")
ROUTE_KEYS = ("pairs", "small", "single", "wg", "duo", "overlap", "share", "kernels")


def parse_routes(text):
    out = []
    for m in ROUTE.finditer(text):
        g = m.groups()
        out.append(dict(zip(ROUTE_KEYS, [int(v) for v in g[:6]] + [g[6], g[7]])))
    return out


def line_of(p):
    return {k: p[k] for k in ROUTE_KEYS}


def want_flags(p, kind):
    """(mask, value) per pair of a planned list: the bits of the flags word that the route fixes."""
    n = p["pairs"]
    mask = np.full(n, FLAG_SINGLE | FLAG_WORKGROUP | FLAG_FAST, dtype=np.uint32)
    val = np.where(p["single_mask"], FLAG_SINGLE, 0).astype(np.uint32) | np.where(p["wg_mask"], FLAG_WORKGROUP, 0).astype(np.uint32)
    if kind == "fast":
        val |= FLAG_FAST
    else:
        mask |= FLAG_INTEGER
        if kind == "int":
            val |= FLAG_INTEGER
    return mask, val


# ---------------------------------------------------------------- the oracle's answers
def best_rule(q, t, f, status, tc, k, f_min=float("-inf")):
    """aln_best_rules.h, as tests/test_best_gpu.py restates it: per row of tc pairs the pairs that succeeded with f >= f_min by
    descending f (-0.0 == +0.0), equal f by ascending target, the first k; then all of them in ascending pair order."""
    ok = (status == 0) & (f == f) & (f >= f_min)
    kept = []
    for r in range(len(f) // tc):
        idx = r * tc + np.flatnonzero(ok[r * tc:(r + 1) * tc])
        kept.append(idx[np.lexsort((t[idx], -(f[idx] + 0.0)))][:k])
    return np.sort(np.concatenate(kept)).astype(np.int64) if kept else np.zeros(0, dtype=np.int64)


def expected(orc, b, threads=16):
    """The oracle's answer of every pair of a block: status and f per pair; of the pairs that succeeded (the held hits at
    f_min = -inf, in pair order) every summary field and both strings."""
    codes, L = set_codes(), set_lengths()
    off = np.concatenate([[0], np.cumsum(L)[:-1]]).astype(np.uint64)
    q, t = b.pairs()
    S, dele, ext, _ = schemes()[b.scheme]
    ref, tb, _ = orc.align_batch(b.semantics, np.concatenate(codes), off[q], L[q].astype(np.uint64), off[t], L[t].astype(np.uint64), dele, ext, S,
                                 n_threads=threads)
    r = np.frombuffer(ref, dtype=ch.ORC_DTYPE)
    ok = r["status"] == 0
    want = dict(pair_status=r["status"].copy(), pair_f=np.where(ok, r["f"], 0.0), index=np.flatnonzero(ok).astype(np.uint64))
    for name in SUMMARY:
        want[name] = r[name][ok].copy()
    idx = ch.string_index(L[q].astype(np.uint64), L[t].astype(np.uint64), np.where(ok, r["aln_len"], 0))
    want["strings"] = tb[idx]
    return want


def subset(want, keep):
    """The held answer of the listed positions of a block's successful pairs (a best pass holds some of them)."""
    pos = np.searchsorted(want["index"], keep)
    assert np.array_equal(want["index"][pos], np.asarray(keep, dtype=np.uint64))
    out = {name: want[name][pos] for name in SUMMARY}
    out["index"] = want["index"][pos]
    ends = np.cumsum(2 * want["aln_len"].astype(np.int64))
    parts = [want["strings"][ends[p] - 2 * int(want["aln_len"][p]):ends[p]] for p in pos]
    out["strings"] = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return out


# ---------------------------------------------------------------- the child processes of tests/test_set_routes_gpu.py
def mark(label):
    """A line on stderr in front of a call: the parent cuts the library's `aln route:` lines by it."""
    sys.stderr.flush()
    os.write(2, ("route call: %s\n" % label).encode())


def cut_by_call(stderr):
    """label -> the route lines printed between its marker and the next one."""
    out, parts = {}, re.split(r"^route call: (\S+)\n", stderr, flags=re.M)
    for label, text in zip(parts[1::2], parts[2::2]):
        assert label not in out, label
        out[label] = parse_routes(text)
    return out


def held_got(held):
    res, strs = held.strings()
    got = {name: res[name] for name in SUMMARY}
    got["index"] = held.index
    got["strings"] = np.concatenate([np.concatenate(p) for p in strs]) if strs else np.zeros(0, np.uint8)
    got["_flags"] = res["flags"]
    return got


def digest(got):
    h = hashlib.sha256()
    for name in ("index",) + tuple(SUMMARY) + ("strings",):
        h.update(np.ascontiguousarray(got[name]).tobytes())
    return h.hexdigest()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def score_diff(f, status, want):
    if not np.array_equal(status, want["pair_status"]):
        return "status differs at pair %d" % int(np.argmax(status != want["pair_status"]))
    if not np.array_equal(_bits(f), _bits(want["pair_f"])):
        return "f differs at pair %d" % int(np.argmax(_bits(f) != _bits(want["pair_f"])))
    return None


def _held_call(calls, label, run, want):
    import time
    mark(label)
    t0 = time.perf_counter()
    got = held_got(run())
    want = {k: v for k, v in want.items() if not k.startswith("pair_")}
    calls.append(dict(label=label, diff=ch.compare(got, want), flags=[int(v) for v in got["_flags"]], digest=digest(got),
                      seconds=time.perf_counter() - t0))


def _score_call(calls, label, run, want):
    import time
    mark(label)
    t0 = time.perf_counter()
    f, status = run()
    h = hashlib.sha256(np.ascontiguousarray(f).tobytes() + np.ascontiguousarray(status).tobytes()).hexdigest()
    calls.append(dict(label=label, diff=score_diff(f, status, want), flags=None, digest=h, seconds=time.perf_counter() - t0))


def best_want(b, want, k=2):
    q, t = b.pairs()
    return subset(want, best_rule(q, t, want["pair_f"], want["pair_status"], b.tn, k))


def run_block(ss, b, want, calls, candidates=True, tag=""):
    """Every pass of one block: score, hits at -inf with strings, best (rectangles: an upper block has no rows), then the same
    over the candidate list of a prefilter that keeps every pair (duo and overlap: the candidate score pass only)."""
    S, dele, ext, _ = schemes()[b.scheme]
    kw, blk, name = dict(semantics=b.semantics), b.tuple(), tag + b.name
    _score_call(calls, name + "/score", lambda: ss.score(S, dele, ext, blk, **kw), want)
    _held_call(calls, name + "/hits", lambda: ss.hits(S, dele, ext, float("-inf"), blk, **kw), want)
    if not b.upper:
        _held_call(calls, name + "/best", lambda: ss.best(S, dele, ext, 2, block=blk, **kw), best_want(b, want))
    if not candidates:
        return
    mark(name + "/prefilter")
    cand = ss.prefilter(KMER[0], KMER[1], 0, 0, blk)
    assert len(cand) == len(want["pair_status"]) and np.array_equal(cand.index, np.arange(len(cand), dtype=np.uint64))
    _score_call(calls, name + "/cand_score", lambda: cand.score(S, dele, ext, **kw), want)
    if b.name in ("duo", "overlap"):
        return
    _held_call(calls, name + "/cand_hits", lambda: cand.hits(S, dele, ext, float("-inf"), **kw), want)
    if not b.upper:
        _held_call(calls, name + "/cand_best", lambda: cand.best(S, dele, ext, 2, **kw), best_want(b, want))


def _child_passes(wants, only):
    from aligner_amd.seqset import SeqSet
    calls = []
    with SeqSet(set_codes()) as ss:
        for b in blocks():
            if only in (None, b.name):
                run_block(ss, b, wants[b.name], calls, candidates=only is None)
    return dict(calls=calls)


def schedule_names():
    return [blocks()[i].name for i in ch.schedule(SCHEDULE_BLOCKS)]


def _child_schedule(wants, between):
    """hits at -inf plus strings, block after block in the order of call_history.schedule(8), on one set; between: a score pass of
    the previous block in front of every call but the first (a device-expanded pass between two held passes)."""
    from aligner_amd.seqset import SeqSet
    calls, prev = [], None
    with SeqSet(set_codes()) as ss:
        for step, name in enumerate(schedule_names()):
            b = block(name)
            S, dele, ext, _ = schemes()[b.scheme]
            if between and prev is not None:
                pS, pd, pe, _ = schemes()[prev.scheme]
                _score_call(calls, "%d/%s/between" % (step, prev.name), lambda: ss.score(pS, pd, pe, prev.tuple(), semantics=prev.semantics),
                            wants[prev.name])
            _held_call(calls, "%d/%s/hits" % (step, name), lambda: ss.hits(S, dele, ext, float("-inf"), b.tuple(), semantics=b.semantics),
                       wants[name])
            prev = b
    return dict(calls=calls)


def main(argv):
    mode, expected_path, report = argv[:3]
    only = argv[3] if len(argv) > 3 else None
    wants = ch.load_expected(expected_path)
    if mode == "passes":
        out = _child_passes(wants, only)
    else:
        out = _child_schedule(wants, mode == "schedule_between")
    with open(report, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1:])
