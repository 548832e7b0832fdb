"""The cases of tests/test_plan_rules_cpu.py: lists of pair lengths, the call's scheme and the plan's knobs, the smallest at which each
rule of the batch plan (aligner_amd/csrc/aln_plan_rules.h) turns.  Not a test module.  A case names its lengths by a short spec
(lengths()), so that tests/golden/plan_cases.json holds specs, knobs and recorded results only; case_line() writes a case for
tests/plan_rules_driver.cpp."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import route_cases as rc  # noqa: E402
from aligner_amd import workloads  # noqa: E402
from aligner_amd.distributed import lpt_shards  # noqa: E402

CUS = 256
PWM_LOCAL = 4
PWM_COLS = 12
BASE_ENV = {k: v for k, v in rc.CHILD_ENV.items() if k != "ALN_TRACE_PLAN"}       # read once per process: not a case's knob
FACTS = ("pwm", "fast", "is_int", "want_h", "want_tb", "store_dirs", "semantics", "rows", "cols", "hazard", "force_serial", "pair_matrices")
SCALARS = ("first", "n", "n_small", "cells", "max_cells", "dir_bytes", "tb_bytes", "tag_bytes", "hmat_elems", "max_len", "grid", "zrow_bytes",
           "lds_bytes", "prof_stride", "tb_waves", "single_max_n", "cascade_rows", "duo_qo", "scratch_stride", "granule_bytes", "tbmap_entries",
           "granule_stride_max", "counter_bytes", "overlap", "coop", "coop_linger", "coop_lean", "coop_tail", "coop_bytes", "seq_direct", "seq_lo",
           "seq_span", "h_descs", "h_order", "h_single_pairs", "h_single_r", "h_wg_pairs", "h_wg_r", "n_single", "n_wg", "need_seq_span", "need_n",
           "need_dir_bytes", "need_tb_bytes", "need_tag_bytes", "need_scratch", "need_coop", "stored_dir_bytes")
FORCED_CELLS = ("250000", "1000000", "4000000")      # the chunkings the GPU tests force with ALN_CHUNK_CELLS


def pair_cost(N, M):
    """aln_pair_cost, restated (as tests/test_coop_lean_cpu.py does)."""
    c, ns = 0, (M + 511) // 512
    for s in range(ns):
        rows = min(M - s * 512, 512)
        R = max(1, min(8, (rows + 63) // 64)) if s + 1 == ns else 8
        c += (N + (rows + R - 1) // R - 1) * (24 + 21 * R)
    return c


# the lean edges of test_coop_lean_cpu.test_rule_edges as lengths: 16 pairs per resident wave, a score pass (1024 workgroups, so the
# tail is the last 8192 queue positions and the share is per resident wave); bulk pairs of 512 x 512, tail pairs of x x 100, and a
# first pair of y x 512
LEAN_W = CUS * 12
LEAN_N = 16 * LEAN_W
LEAN_TAIL = 2 * CUS * 16


def _lean_total(x, y):
    return (LEAN_N - LEAN_TAIL - 1) * pair_cost(512, 512) + LEAN_TAIL * pair_cost(x, 100) + pair_cost(y, 512)


def lean_tail_edge():
    """The largest x for which the tail's longest pair costs at most 1/64 of a wave's share."""
    x = 100
    while pair_cost(x + 1, 100) * 64 * LEAN_W <= _lean_total(x + 1, 512):
        x += 1
    return x


def lean_head_edge():
    """The largest y for which the queue's longest pair costs at most a quarter of a wave's share."""
    y = 512
    while pair_cost(y + 1, 512) * 4 * LEAN_W <= _lean_total(100, y + 1):
        y += 1
    return y


def lengths(spec):
    """(query lengths, target lengths) of a spec: block:NAME:held|score, c5:N, shard, lean:N:X:Y, or N1xM1*count+N2xM2*count..."""
    kind, _, rest = spec.partition(":")
    if kind == "block":
        name, mode = rest.split(":")
        b, L = rc.block(name), rc.set_lengths()
        q, t = b.pairs()
        if mode == "held":
            keep = np.array([rc.LAYOUT[a] != rc.BAD and rc.LAYOUT[c] != rc.BAD for a, c in zip(q, t)])
            q, t = q[keep], t[keep]
        return L[q], L[t]
    if kind == "c5":
        return workloads.c5_lengths(int(rest))
    if kind == "shard":
        q, t = workloads.c5_lengths(100000)
        s = lpt_shards(q * t, 8)[0]
        return q[s], t[s]
    if kind == "lean":
        n, x, y = (int(v) for v in rest.split(":"))
        q = np.full(n, 512, dtype=np.int64)
        t = np.full(n, 512, dtype=np.int64)
        q[0] = y
        q[n - LEAN_TAIL:], t[n - LEAN_TAIL:] = x, 100
        return q, t
    if kind == "mix":                                # equal costs and unequal ones, unsorted
        r = np.random.default_rng(int(rest))
        pick = r.integers(0, 3, 60)
        return np.array([100, 250, 100])[pick], np.array([100, 90, 300])[pick]
    q, t = [], []
    for part in spec.split("+"):
        shape, _, count = part.partition("*")
        N, M = shape.split("x")
        q += [int(N)] * int(count or 1)
        t += [int(M)] * int(count or 1)
    return np.array(q, dtype=np.int64), np.array(t, dtype=np.int64)


def offsets(q, t, scattered=False, pwm=False):
    """Packed: every pair's query, then its target, back to back.  Scattered: every pair a megabyte further on."""
    q_off, t_off, pos = np.zeros(len(q), np.uint64), np.zeros(len(q), np.uint64), 0
    for i, (a, b) in enumerate(zip(q, t)):
        if scattered:
            pos = i << 20
        q_off[i] = 0 if pwm else pos
        pos += 0 if pwm else int(a)
        t_off[i] = pos
        pos += int(b)
    return q_off, t_off


def case(name, spec, scheme="INT", local=True, held=True, env=None, allow=True, many=False, scattered=False, first=0, n=None, want_h=False):
    return dict(want_h=want_h, name=name, spec=spec, scheme=scheme, semantics=PWM_LOCAL if scheme == "PWM" else rc.CORE_LOCAL if local else rc.CORE_GLOBAL,
                held=held, env=dict(BASE_ENV if env is None else env), allow=allow, many=many, scattered=scattered, first=first, n=n)


def scheme(name):
    """(matrix, del, ext)"""
    if name == "PWM":
        r = np.random.default_rng(7)
        return r.integers(-3, 4, (4, PWM_COLS)).astype(np.float64), 3.0, 1.0
    return rc.schemes()[name][:3]


def cases():
    out = []
    # 1. every route's block, held pass and score pass, under the knob variants of test_set_routes_cpu.py
    variants = dict(base=BASE_ENV, no_duo=dict(BASE_ENV, ALN_NO_DUO="1"), no_overlap=dict(BASE_ENV, ALN_TB_OVERLAP="0"),
                    no_any={k: v for k, v in BASE_ENV.items() if k != "ALN_TB_OVERLAP_ANY"}, no_coop=dict(BASE_ENV, ALN_NO_COOP="1"),
                    no_wgpipe=dict(BASE_ENV, ALN_NO_WGPIPE="1"), time_rule={k: v for k, v in BASE_ENV.items() if k != "ALN_BIG_TO_SINGLE"})
    for b in rc.blocks():
        for mode in ("held", "score"):
            for v, env in variants.items():
                out.append(case("block/%s/%s/%s" % (b.name, mode, v), "block:%s:%s" % (b.name, mode), b.scheme, b.local(), mode == "held", env))
    # 2. chunk-size and flag edges
    out += [case("n16", "600x640*16"), case("n17", "600x640*17"), case("real4", "300x130*4", "REAL"), case("real5", "300x130*5", "REAL"),
            case("not_alone/n16", "600x640*16", allow=False), case("not_alone/coop", "block:coop:held", allow=False),
            case("not_alone/overlap", "block:overlap:held", allow=False), case("many_chunks/coop", "block:coop:held", allow=False, many=True)]
    # 3. the single-pair route
    out += [case("single/m2560", "1000x2560"), case("single/m2561", "1000x2561"), case("single/m262144", "64x262144", env=dict(BASE_ENV, ALN_SINGLE_R="1")),
            case("single/m262145", "64x262145", env=dict(BASE_ENV, ALN_SINGLE_R="1")), case("single/n100000", "100000x2000"), case("single/n100001", "100001x2000"),
            case("single/lds_in", "78656x2000"), case("single/lds_out", "78657x2000"),     # 159 KiB of LDS: 24 x 24, one row per lane
            case("single/r3", "600x640", env=dict(BASE_ENV, ALN_SINGLE_R="3")), case("single/off", "600x640", env=dict(BASE_ENV, ALN_NO_SINGLE="1"))]
    # 4. one workgroup per pair
    out += [case("wg/m%d" % M, "300x%d" % M, "REAL") for M in (64, 65, 512, 513, 1024, 1025, 2048, 2049)]
    out += [case("wg/r1_16_strips", "300x1024", "REAL", env=dict(BASE_ENV, ALN_WG_R="1")),
            case("wg/r1_17_strips", "300x1025", "REAL", env=dict(BASE_ENV, ALN_WG_R="1")),
            case("wg/r4", "300x300", "REAL", env=dict(BASE_ENV, ALN_WG_R="4")), case("wg/h_dump", "300x300", "INT", want_h=True)]
    # 5. empty, PWM and scattered inputs
    out += [case("empty/query", "100x100+0x100+100x100"), case("empty/target", "100x100+100x0+100x100"),
            case("empty/pwm_target", "%dx330+%dx0+%dx330" % ((PWM_COLS,) * 3), "PWM"), case("pwm/8", "%dx330*7+%dx200" % (PWM_COLS, PWM_COLS), "PWM"),
            case("scattered", "300x200*6", scattered=True), case("packed", "300x200*6")]
    # 6. sharing
    x, y = lean_tail_edge(), lean_head_edge()
    out += [case("lean/pairs_%d" % n, "lean:%d:100:512" % n, held=False) for n in (LEAN_N - 1, LEAN_N)]
    out += [case("lean/tail_%s" % w, "lean:%d:%d:512" % (LEAN_N, v), held=False) for w, v in (("in", x), ("out", x + 1))]
    out += [case("lean/head_%s" % w, "lean:%d:100:%d" % (LEAN_N, v), held=False) for w, v in (("in", y), ("out", y + 1))]
    out += [case("share/coop_tail", "block:coop:held", env=dict(BASE_ENV, ALN_COOP_TAIL="5")),
            case("share/chain", "4200x4200*256", held=False, env={}), case("share/no_chain", "4200x4200*256", held=False, env=dict(ALN_CHAIN_WGS="0")),
            case("share/fill_wgs", "block:coop:held", env=dict(BASE_ENV, ALN_FILL_WGS="1")),
            case("c5/held", "c5:100000", env={}), case("c5/score", "c5:100000", held=False, env={}), case("c5/shard", "shard", env={})]
    # 7. order: a queue that arrives sorted, one that does not, equal costs
    out += [case("order/sorted", "100x100*1000"), case("order/unsorted", "c5:1000", env={}), case("order/equal", "mix:3")]
    # the forced chunkings of the GPU tests (the bounds of a pipelined call against every chunk's own plan)
    for cells in FORCED_CELLS:
        out += [case("chunks/c5_300/%s" % cells, "c5:300", env=dict(ALN_CHUNK_CELLS=cells)),
                case("chunks/real/%s" % cells, "c5:60", "REAL", env=dict(ALN_CHUNK_CELLS=cells)),
                case("chunks/n17/%s" % cells, "600x640*17", env=dict(BASE_ENV, ALN_CHUNK_CELLS=cells)),
                case("chunks/mixed/%s" % cells, "block:single_mixed:held", env=dict(BASE_ENV, ALN_CHUNK_CELLS=cells)),
                case("chunks/global/%s" % cells, "c5:300", local=False, held=False, env=dict(ALN_CHUNK_CELLS=cells)),
                case("chunks/pwm/%s" % cells, "%dx330*640" % PWM_COLS, "PWM", env=dict(ALN_CHUNK_CELLS=cells))]
    assert len({c["name"] for c in out}) == len(out)
    return out


def tables(c):
    q, t = lengths(c["spec"])
    q_off, t_off = offsets(q, t, c["scattered"], c["scheme"] == "PWM")
    return q_off, np.asarray(q, np.uint64), t_off, np.asarray(t, np.uint64)


def _knob(env, name):
    return "%d %d" % ((1, int(env[name])) if name in env else (0, 0))


def case_line(c, facts, tables_path, lists_path="-"):
    """The driver's line for a case; facts: the call's facts as the fixture holds them (FACTS)."""
    env, n_total = c["env"], len(lengths(c["spec"])[0])
    assert not set(env) - {"ALN_SINGLE_R", "ALN_NO_SINGLE", "ALN_NO_COOP", "ALN_BIG_TO_SINGLE", "ALN_NO_WGPIPE", "ALN_WG_R", "ALN_TB_OVERLAP",
                           "ALN_TB_OVERLAP_ANY", "ALN_COOP_TAIL", "ALN_CHAIN_WGS", "ALN_FILL_WGS", "ALN_NO_DUO", "ALN_CHUNK_CELLS", "ALN_COOP_LEAN"}
    words = [c["name"], str(tables_path), n_total, c["first"], n_total - c["first"] if c["n"] is None else c["n"], int(c["allow"]), int(c["many"]), CUS]
    words += [int(facts[k]) for k in FACTS]
    words += [_knob(env, "ALN_SINGLE_R"), int("ALN_NO_SINGLE" in env), int("ALN_NO_COOP" in env), _knob(env, "ALN_BIG_TO_SINGLE"),
              int("ALN_NO_WGPIPE" in env), _knob(env, "ALN_WG_R"), _knob(env, "ALN_TB_OVERLAP"), int("ALN_TB_OVERLAP_ANY" in env), int(env.get("ALN_COOP_LEAN", -1)),
              _knob(env, "ALN_COOP_TAIL"), _knob(env, "ALN_CHAIN_WGS"), _knob(env, "ALN_FILL_WGS"), int("ALN_NO_DUO" in env),
              "1 %s" % env["ALN_CHUNK_CELLS"] if "ALN_CHUNK_CELLS" in env else "0 0", str(lists_path)]
    return " ".join(str(w) for w in words)


def parse_line(line):
    """name, {key: int | str} of one output line of the driver"""
    name, *words = line.split()
    out = {}
    for w in words:
        k, _, v = w.partition("=")
        out[k] = int(v) if v.lstrip("-").isdigit() else v
    return name, out
