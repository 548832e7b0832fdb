"""Clusters on the device (aln_cluster_edges / aln_seqset_held_cluster, cluster.cluster_edges / HeldHits.cluster) against the plain
Python rules of cluster_ref.py: labels, records and summaries, integer for integer.  Graphs whose shape is chosen directly -- the
degenerate ones, random ones, edge counts around the launch grid, a scrambled path (with the round bound that refuses one hop per
round), the greedy rule's corners, node counts around the compaction's tiles and its second trip -- then capacities, determinism,
the held hits of a sequence set over every kind of block, the refusals, the command and the C99 caller."""
import ctypes as C
import hashlib
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cluster_cases  # noqa: E402
import cluster_ref as R  # noqa: E402
from aligner_amd import _ffi, allpairs, cluster, runtime  # noqa: E402
from aligner_amd import build as native_build  # noqa: E402
from aligner_amd.enums import Protein  # noqa: E402
from aligner_amd.fasta import encode_records, read_fasta  # noqa: E402
from aligner_amd.matrices import get_blosum62  # noqa: E402
from aligner_amd.seqset import SeqSet, rectangle  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (("components", R.COMPONENTS), ("greedy", R.GREEDY))
SUMMARY_KEYS = ("nodes", "clusters", "edges", "self_edges", "singletons")


def tuples(records):
    return [tuple(int(x) for x in r) for r in records.tolist()]


def check(got, mode, n, a, b, lengths=None, nodes=None):
    """a Clusters against the reference's (label, records, summary, members)"""
    lab, recs, summ, mem = R.cluster(mode, n, a, b, lengths, nodes)
    assert got.label.dtype == np.uint32 and got.label.tolist() == lab
    assert got.records.dtype == cluster.RECORD_DTYPE and tuples(got.records) == recs
    assert {k: got.summary[k] for k in SUMMARY_KEYS} == summ
    assert [m.tolist() for m in got.members()] == mem
    return lab, recs, summ


def both(n, a, b, lengths=None):
    out = []
    for name, mode in MODES:
        got = cluster.cluster_edges(n, a, b, lengths, mode=name)
        check(got, mode, n, a, b, lengths)
        out.append(got)
    return out


# ---------------------------------------------------------------- graphs of a chosen shape
def test_degenerate_graphs():
    for name, mode in MODES:
        got = cluster.cluster_edges(0, [], [], mode=name)
        assert len(got.label) == 0 and len(got.records) == 0 and got.summary == dict(nodes=0, clusters=0, edges=0, self_edges=0, singletons=0, rounds=0)
    both(1, [], [])
    both(1, [0, 0], [0, 0])                                        # only self edges
    both(7, [], [], [3, 3, 1, 9, 9, 0, 2])                         # no edges
    both(5, [2, 4, 0], [2, 4, 0])
    c, g = both(6, [4, 1, 4, 1, 4], [1, 4, 1, 4, 1], [1, 1, 1, 1, 5, 1])      # one edge listed five times, both orientations
    assert tuples(c.records)[1] == (1, 2, 4, 5) and tuples(g.records)[3] == (4, 2, 4, 5)


def test_random_graphs():
    rng = np.random.default_rng(20251)
    for _ in range(300):
        n = int(rng.integers(1, 41))
        m = int(rng.integers(0, 61))
        a = rng.integers(0, n, size=m).astype(np.uint32)
        b = rng.integers(0, n, size=m).astype(np.uint32)            # self edges and duplicates happen
        if m > 4:
            a[-1], b[-1] = b[0], a[0]                               # one edge again, the other way round
        lengths = rng.integers(0, 4, size=n).astype(np.uint32) if rng.random() < 0.7 else None      # many ties
        both(n, a, b, lengths)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 2048, 2049])
def test_edge_counts_around_the_grid(m):
    rng = np.random.default_rng(m)
    n = 100
    a = rng.integers(0, n, size=m).astype(np.uint32)
    b = rng.integers(0, n, size=m).astype(np.uint32)
    a[-1], b[-1] = 98, 99                                            # the last edge of the list counts
    both(n, a, b, rng.integers(0, 6, size=n).astype(np.uint32))


def test_a_scrambled_path_settles_in_few_rounds():
    """4 097 nodes in a path under a fixed permutation.  One hop per round would need about 4 096 rounds; hook and compress halve the
    trees: about ceil(log2 4 097) + 1 = 14.  Observed on an MI355X: 9 rounds."""
    n = 4097
    a, b = cluster_cases.scrambled_path(n)
    got = cluster.cluster_edges(n, a, b, mode="components")
    print("scrambled path: rounds", got.summary["rounds"])
    assert got.label.tolist() == [0] * n
    assert tuples(got.records) == [(0, n, 0, n - 1)]
    assert got.summary["clusters"] == 1 and got.summary["edges"] == n - 1 and got.summary["singletons"] == 0
    assert got.summary["rounds"] <= 64


def test_greedy_cases():
    # a star whose hub is the shortest node: the longest leaf represents the hub, every other leaf itself; components: one cluster
    n = 9
    lengths = [1, 10, 12, 30, 12, 11, 10, 10, 10]                    # hub 0; leaf 3 is the longest
    a, b = [0] * (n - 1), list(range(1, n))
    c, g = both(n, a, b, lengths)
    assert g.label.tolist() == [3, 1, 2, 3, 4, 5, 6, 7, 8] and tuples(g.records)[2] == (3, 2, 3, 1)
    assert c.label.tolist() == [0] * n and tuples(c.records) == [(0, n, 3, n - 1)]
    # a member adjacent to two representatives takes the earlier in priority order (here the higher number)
    c, g = both(4, [0, 3, 1], [2, 2, 1], [5, 1, 2, 9])
    assert g.label.tolist() == [0, 1, 3, 3]
    # equal lengths tie by index: with no lengths at all, and with equal ones
    for lengths in (None, [4, 4, 4, 4, 4]):
        c, g = both(5, [4, 3, 2, 1], [3, 2, 1, 0], lengths)
        assert g.label.tolist() == [0, 0, 2, 2, 4]
    # a path with lengths descending along it: node i is decided in round i + 1
    n = 513
    a, b = np.arange(n - 1, dtype=np.uint32), np.arange(1, n, dtype=np.uint32)
    c, g = both(n, a, b, np.arange(n, 0, -1).astype(np.uint32) + 1000)
    print("descending path: rounds", g.summary["rounds"])
    assert g.label.tolist() == [i - (i & 1) for i in range(n)]
    assert g.summary["rounds"] <= n + 2


@pytest.mark.parametrize("n", [2047, 2048, 2049])
def test_node_counts_around_a_tile(n):
    a = [2046, 0, 5, 2040]
    b = [2045, 2046, 5, 1]
    if n > 2047:
        a += [2047, 2047]
        b += [2046, 3]
    if n > 2048:
        a += [2047, 2048]
        b += [2048, 9]                                               # across 2047 | 2048
    both(n, a, b)


def test_the_compaction_second_trip():
    """524 289 + 2 048 nodes: more than 256 tiles, so the shared offsets kernel makes a second trip.  Tile 3 holds no label (a star
    from node 0), every node of tile 5 is the label of a pair whose other end fills tile 6, every other tile is all singletons or
    nearly; the edge {524 287, 524 288} joins the last node of tile 255 and the first of tile 256."""
    n = 524289 + 2048
    t = 2048
    star = np.arange(3 * t, 4 * t, dtype=np.uint32)
    pair = np.arange(5 * t, 6 * t, dtype=np.uint32)
    a = np.concatenate([np.zeros(t, dtype=np.uint32), pair, [524287, 2047, n - 1, 300000]]).astype(np.uint32)
    b = np.concatenate([star, pair + t, [524288, 2048, n - 2, 300000]]).astype(np.uint32)
    al, bl = a.tolist(), b.tolist()
    for name, mode in MODES:
        got = cluster.cluster_edges(n, a, b, mode=name)
        lab, recs, summ, _mem = R.cluster(mode, n, al, bl)
        assert np.array_equal(got.label, np.array(lab, dtype=np.uint32))
        assert got.records.tobytes() == np.array(recs, dtype=np.uint32).tobytes()          # the whole cluster list
        assert {k: got.summary[k] for k in SUMMARY_KEYS} == summ
        assert summ["clusters"] == n - t - t - 3 and not (set(range(3 * t, 4 * t)) | set(range(6 * t, 7 * t))) & set(lab)


# ---------------------------------------------------------------- capacity, determinism
def raw_edges(n, a, b, mode, capacity, lengths=None, fill=0x5A):
    lib = _ffi.load()
    a, b = np.ascontiguousarray(a, dtype=np.uint32), np.ascontiguousarray(b, dtype=np.uint32)
    label = np.zeros(n, dtype=np.uint32)
    rec = np.full(16 * (capacity + 2), fill, dtype=np.uint8)          # two records of guard behind the capacity
    summ = _ffi.ClusterSummary()
    st = lib.aln_cluster_edges(runtime.context(None), mode, n, lengths.ctypes.data if lengths is not None else None, a.ctypes.data, b.ctypes.data, len(a),
                               label.ctypes.data, rec.ctypes.data, capacity, C.byref(summ))
    assert st == 0
    return label, rec, summ


def test_capacities():
    rng = np.random.default_rng(8)
    n, m = 300, 200
    a, b = rng.integers(0, n, size=m).astype(np.uint32), rng.integers(0, n, size=m).astype(np.uint32)
    lengths = rng.integers(0, 5, size=n).astype(np.uint32)
    for name, mode in MODES:
        lab, recs, summ, _mem = R.cluster(mode, n, a.tolist(), b.tolist(), lengths.tolist())
        count = len(recs)
        assert count > 3
        for cap in (0, count - 1, count, count + 5):
            label, rec, s = raw_edges(n, a, b, mode, cap, lengths)
            wrote = min(cap, count)
            assert label.tolist() == lab and s.clusters == count and s.singletons == summ["singletons"]
            assert rec[:16 * wrote].tobytes() == np.array(recs[:wrote], dtype=np.uint32).tobytes()
            assert rec[16 * wrote:].tobytes() == bytes([0x5A]) * (16 * (cap + 2 - wrote))


def test_the_same_bytes_whatever_the_order():
    rng = np.random.default_rng(77)
    n, m = 5000, 7000
    a, b = rng.integers(0, n, size=m).astype(np.uint32), rng.integers(0, n, size=m).astype(np.uint32)
    lengths = rng.integers(0, 9, size=n).astype(np.uint32)
    perm = rng.permutation(m)
    for _name, mode in MODES:
        def state(x, y):
            label, rec, s = raw_edges(n, x, y, mode, n, lengths)
            return label.tobytes(), rec.tobytes(), bytes(s)
        first = state(a, b)
        assert state(a, b) == first                                  # a second call on the same context
        assert state(b[perm], a[perm]) == first                      # permuted, the other way round
        assert state(a[::-1], b[::-1]) == first


# ---------------------------------------------------------------- the held hits of a sequence set
F_MIN = 200.0                 # hits: at this threshold the set falls into families and loners (checked with the CPU oracle)
FILTER = dict(min_identity=0.5, min_q_cover=0.5)


@pytest.fixture(scope="module")
def families():
    S = get_blosum62()
    codes, family = cluster_cases.family_set()
    with SeqSet(codes) as ss:
        yield ss, codes, S


def held_edges(held, S, th):
    """the edges the existing calls give: held_list, and with thresholds the filter's positions"""
    if th is None:
        return held.q.tolist(), held.t.tolist(), len(held)
    pos = held.filter(S, **th)
    return held.q[pos].tolist(), held.t[pos].tolist(), len(pos)


def check_held(ss, held, S, nodes, vacuous=True):
    n = len(ss)
    lens = ss.len.tolist()
    for th in (None, FILTER):
        a, b, kept = held_edges(held, S, th)
        if th is not None and vacuous:
            assert 0 < kept < len(held)                              # the filter removes some edges, not all
        for name, mode in MODES:
            got = held.cluster(S if th else None, mode=name, **(th or {}))
            lab, recs, summ = check(got, mode, n, a, b, lens, nodes)
            st = ss.stats()
            assert st["bytes_up"] == 8 * len(held) + (4 * ((S.size + 31) // 32) if th else 0)
            assert st["bytes_down"] == 4 * n + 16 * len(recs) + 32 + 4 * got.summary["rounds"]
            if th is not None and vacuous:
                assert sum(1 for r in recs if r[1] >= 2) >= 3 and summ["singletons"] >= 1


def test_held_hits_of_the_upper_block(families):
    ss, codes, S = families
    held = ss.hits(S, 11, 2, F_MIN, None)
    assert len(held) > 0
    check_held(ss, held, S, None)
    # without thresholds too the set is more than one family
    got = held.cluster(mode="components")
    assert sum(1 for r in tuples(got.records) if r[1] >= 2) >= 3 and got.summary["singletons"] >= 1


def test_held_hits_of_the_k_best(families):
    ss, codes, S = families
    held = ss.best(S, 11, 2, 3, skip_self=True)
    assert len(held) == 3 * len(ss)
    check_held(ss, held, S, None)


def test_a_rectangle_and_one_against_many(families):
    ss, codes, S = families
    n = len(ss)
    held = ss.hits(S, 11, 2, 60.0, rectangle(5, 10, 20, 30))
    nodes = list(range(5, 15)) + list(range(20, 50))
    assert len(held) > 0
    check_held(ss, held, S, nodes, vacuous=False)
    got = held.cluster(mode="greedy")
    assert [v for v in range(n) if got.label[v] != cluster.NONE] == nodes and got.summary["nodes"] == 40
    # sequence 7 against every sequence, itself included: a self edge
    held = ss.hits(S, 11, 2, 150.0, rectangle(7, 1, 0, n))
    assert 7 in held.t.tolist()
    check_held(ss, held, S, None, vacuous=False)
    assert held.cluster(mode="components").summary["self_edges"] == 1
    # touching ranges: the nodes are their union
    held = ss.best(S, 11, 2, 2, block=rectangle(10, 5, 15, 5))
    check_held(ss, held, S, list(range(10, 20)), vacuous=False)


def digest(held):
    lst = held.__class__(held.owner, len(held), held.semantics)       # (held_list again)
    res, strs = held.strings()
    h = hashlib.sha256()
    for part in (lst.index, lst.q, lst.t, lst.f, res):
        h.update(part.tobytes())
    for x, y in strs:
        h.update(x.tobytes())
        h.update(y.tobytes())
    return h.hexdigest()


def test_held_state_and_call_history(families):
    ss, codes, S = families
    held = ss.hits(S, 11, 2, F_MIN, None)
    before = digest(held)
    rep_before = held.report(S).tobytes()
    s0 = ss.stats()
    first = held.cluster(S, mode="greedy", **FILTER)
    s1 = ss.stats()
    assert (s1["fill_ms"], s1["refill_ms"]) == (s0["fill_ms"], s0["refill_ms"]) and s1["fetch_kernel_ms"] >= 0 and s1["wall_ms"] > 0
    # another call on the same context in between: an edge list of its own, in the other mode
    cluster.cluster_edges(500, np.arange(499), np.arange(1, 500), mode="components")
    again = held.cluster(S, mode="greedy", **FILTER)
    assert again.label.tobytes() == first.label.tobytes() and again.records.tobytes() == first.records.tobytes() and again.summary == first.summary
    held.cluster(mode="components")
    assert digest(held) == before and held.report(S).tobytes() == rep_before


def test_a_real_valued_scheme(families):
    """the filter's scheme is the caller's: the reports are classed under it (its positive bit), as held_filter does"""
    ss, codes, S = families
    held = ss.hits(S, 11, 2, F_MIN, None)
    T = S * 0.37 - 0.11
    a, b, kept = held_edges(held, T, FILTER)
    assert 0 < kept < len(held)
    for name, mode in MODES:
        check(held.cluster(T, mode=name, **FILTER), mode, len(ss), a, b, ss.len.tolist())
    pos, rep = held.filter(T, with_reports=True, **FILTER)
    assert rep.tobytes() == held.report(T, keep=pos).tobytes() and rep.tobytes() != held.report(S, keep=pos).tobytes()


def test_refusals_leave_everything_as_it_was(families):
    ss, codes, S = families
    lib = ss.lib
    n = len(ss)
    held = ss.hits(S, 11, 2, F_MIN, None)
    before = digest(held)
    stats = ss.stats()
    p, _alive = runtime.make_params(_ffi.CORE_LOCAL, 0.0, 0.0, S)
    label = np.full(n, 7, dtype=np.uint32)
    rec = np.full(16 * n, 7, dtype=np.uint8)
    summ = _ffi.ClusterSummary(9, 9, 9, 9, 9, 9, 9)
    flt = _ffi.HitFilter(0.5, 0.0, 0.0, 0, 0)
    INV, UNS = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED

    def call(params=p, flags=1, f=flt, mode=0, lab=label, out=rec, cap=n, s=summ):
        return lib.aln_seqset_held_cluster(ss.handle, C.byref(params) if params is not None else None, flags, C.byref(f) if f is not None else None, mode,
                                           lab.ctypes.data if lab is not None else None, out.ctypes.data if out is not None else None, cap,
                                           C.byref(s) if s is not None else None)

    pwm = _ffi.Params.from_buffer_copy(bytes(p))
    pwm.semantics = _ffi.PWM_LOCAL
    no_matrix = _ffi.Params.from_buffer_copy(bytes(p))
    no_matrix.matrix = None
    assert call(mode=2) == INV and call(mode=0xFFFFFFFF) == INV and call(mode=2, f=None, params=None) == INV
    assert call(flags=2) == INV and call(flags=3) == INV
    assert call(f=_ffi.HitFilter(0.0, 0.0, 0.0, 0, 1)) == INV
    assert call(lab=None) == INV and call(s=None) == INV and call(out=None) == INV
    assert call(params=None) == INV and call(params=no_matrix) == INV
    assert call(params=pwm) == UNS
    assert label.tolist() == [7] * n and rec.tobytes() == bytes([7]) * (16 * n)
    assert (summ.nodes, summ.clusters, summ.edges, summ.self_edges, summ.singletons, summ.rounds, summ.reserved) == (9,) * 7
    assert ss.stats() == stats and digest(held) == before
    assert call(out=None, cap=0) == 0 and summ.reserved == 0 and summ.nodes == n      # no records asked for
    label.fill(7)
    # an edge list of the caller's: an endpoint that is not a node, too many nodes
    e = np.array([0, 5], dtype=np.uint32)
    summ2 = _ffi.ClusterSummary(9, 9, 9, 9, 9, 9, 9)
    lab5 = np.full(5, 7, dtype=np.uint32)
    ctx = runtime.context(None)
    assert lib.aln_cluster_edges(ctx, 0, 5, None, e.ctypes.data, e.ctypes.data, 2, lab5.ctypes.data, None, 0, C.byref(summ2)) == INV
    assert lib.aln_cluster_edges(ctx, 0, 0xFFFFFFF1, None, None, None, 0, lab5.ctypes.data, None, 0, C.byref(summ2)) == INV
    assert lib.aln_cluster_edges(ctx, 0, 5, None, None, e.ctypes.data, 2, lab5.ctypes.data, None, 0, C.byref(summ2)) == INV
    assert lib.aln_cluster_edges(ctx, 0, 5, None, e.ctypes.data, e.ctypes.data, 1, lab5.ctypes.data, None, 3, C.byref(summ2)) == INV
    assert lab5.tolist() == [7] * 5 and summ2.nodes == 9 and summ2.rounds == 9
    # no held state: a score pass replaces it
    ss.score(S, 11, 2, rectangle(0, 2, 0, 2))
    assert call() == INV and call(f=None, params=None) == INV
    assert label.tolist() == [7] * n


# ---------------------------------------------------------------- the command, and the C99 caller
def rows_of(capsys, argv):
    assert allpairs.main(argv) == 0
    return capsys.readouterr().out.splitlines()


def test_the_command(capsys):
    path = os.path.join(ROOT, "tests", "golden", "protein.fasta")
    records = read_fasta(path)
    heads = [r.head.decode("utf-8", "replace") for r in records]
    codes = encode_records(records, Protein)
    S = get_blosum62()

    def rows(got):
        size = {int(r["label"]): int(r["size"]) for r in got.records}
        return ["%s,%s,%d" % (heads[i], heads[l], size[l]) for i, l in enumerate(got.label.tolist()) if l != cluster.NONE]

    with SeqSet(codes) as ss:
        hits = ss.hits(S, 11.0, 2.0, 30.0, None)
        assert len(hits) > 0
        plain_hits = ["%s,%s,%r" % (heads[int(q)], heads[int(t)], float(f)) for q, t, f in zip(hits.q, hits.t, hits.f)]
        got = hits.cluster(mode="components")
        check(got, R.COMPONENTS, len(ss), hits.q.tolist(), hits.t.tolist(), ss.len.tolist())
        want_components = rows(got)
        pos = hits.filter(S, min_identity=0.3)
        got = hits.cluster(S, mode="greedy", min_identity=0.3)
        check(got, R.GREEDY, len(ss), hits.q[pos].tolist(), hits.t[pos].tolist(), ss.len.tolist())
        want_greedy = rows(got)
        best = ss.best(S, 11.0, 2.0, 3, skip_self=True)
        plain_best = ["%s,%d,%s,%r" % (heads[q], int(best.rank[p]) + 1, heads[int(best.t[p])], float(best.f[p])) for q, ps in best.by_query() for p in ps]
        want_best = rows(best.cluster(S, mode="greedy", min_q_cover=0.5))
    assert len(want_components) == len(heads)
    assert rows_of(capsys, ["-i", path, "--f-min", "30", "--cluster", "components"]) == want_components
    assert rows_of(capsys, ["-i", path, "--f-min", "30", "--cluster", "greedy", "--min-identity", "0.3"]) == want_greedy
    assert rows_of(capsys, ["-i", path, "--best", "3", "--cluster", "greedy", "--min-q-cover", "0.5"]) == want_best
    # without the flag: what the command printed before
    assert rows_of(capsys, ["-i", path, "--f-min", "30"]) == plain_hits
    assert rows_of(capsys, ["-i", path, "--best", "3"]) == plain_best
    for bad in (["--cluster", "greedy"], ["--f-min", "30", "--cluster", "greedy", "--report"], ["--cluster", "components", "--heuristic", "--kd", "1", "--r-squared", "1"]):
        with pytest.raises(SystemExit):
            allpairs.main(["-i", path] + bad)
    capsys.readouterr()


def hexd(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def test_through_c(families, tmp_path):
    """tests/abi_cluster.c: both exports called from C99 on buffers of exactly the documented sizes, each followed by a guard zone"""
    ss, codes, S = families
    rng = np.random.default_rng(31)
    n, m = 50, 70
    a, b = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    lengths = rng.integers(0, 4, size=n)
    capacity = 11
    words = [n, 1] + lengths.tolist() + [m] + [int(x) for pair in zip(a, b) for x in pair] + [capacity]
    words += [len(codes)] + [len(c) for c in codes] + [int(x) for c in codes for x in c]
    words += [S.shape[0], S.shape[1]] + [hexd(x) for x in S.ravel()] + [hexd(11.0), hexd(2.0), hexd(F_MIN), 98, hexd(FILTER["min_identity"]), hexd(FILTER["min_q_cover"])]
    case = tmp_path / "case.txt"
    case.write_text(" ".join(str(w) for w in words) + "\n")
    exe = native_build.build_cluster_harness()
    out = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines()]
    assert lines[-1] == ["guards", "ok"]
    blocks = []                                                       # (what, mode, label, records, summary) per call
    for k, l in enumerate(lines):
        if l[0] == "rc":
            assert l[3] == "0", " ".join(l)
            if l[1] in ("cluster_edges", "held_cluster", "held_cluster_filter"):
                lab, rec, summ = lines[k + 1], lines[k + 2], lines[k + 3]
                assert (lab[0], rec[0], summ[0]) == ("label", "records", "summary")
                flat = [int(x) for x in rec[1:]]
                blocks.append((l[1], int(l[2]), [int(x) for x in lab[1:]], [tuple(flat[i:i + 4]) for i in range(0, len(flat), 4)], [int(x) for x in summ[1:]]))
    assert [(w, mo) for w, mo, _l, _r, _s in blocks] == [(w, mo) for w in ("cluster_edges", "held_cluster", "held_cluster_filter") for mo in (0, 1)]
    held = ss.hits(S, 11, 2, F_MIN, None)
    assert ["held", str(len(held))] in lines
    for what, mode, lab, rec, summ in blocks:
        name = MODES[mode][0]
        if what == "cluster_edges":
            want = R.cluster(mode, n, a.tolist(), b.tolist(), lengths.tolist())
            py = cluster.cluster_edges(n, a, b, lengths.astype(np.uint32), mode=name)
            shown = capacity
        else:
            th = FILTER if what == "held_cluster_filter" else None
            ea, eb, _kept = held_edges(held, S, th)
            want = R.cluster(mode, len(ss), ea, eb, ss.len.tolist())
            py = held.cluster(S if th else None, mode=name, **(th or {}))
            shown = len(ss)
        assert lab == want[0] == py.label.tolist()
        assert rec == want[1][:shown] == tuples(py.records)[:shown]
        assert summ[:5] == [want[2][k] for k in SUMMARY_KEYS] == [py.summary[k] for k in SUMMARY_KEYS]
        assert summ[5] == py.summary["rounds"] and summ[6] == 0
