"""The clustering rules without a GPU: aligner_amd/csrc/aln_cluster_rules.h driven through a small C++ program and compared with
cluster_ref.py; cluster_ref.py against a breadth-first restatement of both rules on every graph of up to five nodes and on random
ones; the companion header include/aligner_hip_cluster.h against its mirrors (_ffi.CLUSTER_EXPORTS, the ctypes classes,
tests/abi_cluster.c); and the refusals that need no device."""
import ctypes as C
import itertools
import os
import random
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cluster_ref as R  # noqa: E402
from aligner_amd import _ffi  # noqa: E402
from aligner_amd import build as native_build  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "aln_cluster_rules.h"
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "before")) {         // lines `len_u u len_v v` -> before(u, v) before(v, u) key(u) key(v) index(key(u))
        uint32_t lu, u, lv, v;
        while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &lu, &u, &lv, &v) == 4)
            printf("%d %d %" PRIu64 " %" PRIu64 " %" PRIu32 "\n", (int)aln_cluster_before(lu, u, lv, v), (int)aln_cluster_before(lv, v, lu, u),
                   aln_cluster_key(lu, u), aln_cluster_key(lv, v), aln_cluster_key_index(aln_cluster_key(lu, u)));
        return 0;
    }
    if (!strcmp(argv[1], "nodes")) {          // lines `q_first q_count t_first t_count upper n` -> count, then is_node of 0 .. n - 1
        uint64_t qf, qc, tf, tc, up, n;
        while (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &qf, &qc, &tf, &tc, &up, &n) == 6) {
            aln_seqset_block b;
            b.q_first = qf; b.q_count = qc; b.t_first = tf; b.t_count = tc; b.upper = (uint32_t)up; b.reserved = 0;
            const aln_cluster_nodes r = aln_cluster_nodes_of_block(b);
            printf("%" PRIu64, aln_cluster_node_count(r));
            for (uint64_t v = 0; v < n; ++v) printf(" %d", (int)aln_cluster_is_node(r, v));
            printf("\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "all")) {            // `n` -> count and is_node of 0 .. n + 2 for an edge list's own nodes
        uint64_t n;
        while (scanf("%" SCNu64, &n) == 1) {
            const aln_cluster_nodes r = aln_cluster_nodes_all(n);
            printf("%" PRIu64, aln_cluster_node_count(r));
            for (uint64_t v = 0; v < n + 3; ++v) printf(" %d", (int)aln_cluster_is_node(r, v));
            printf("\n");
        }
        return 0;
    }
    return 2;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")
    tmp = tmp_path_factory.mktemp("cluster_rules")
    src = os.path.join(str(tmp), "drv.cpp")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(str(tmp), "drv")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "aligner_amd", "csrc"), src, "-o", exe])
    return exe


def run(drv, what, lines):
    return subprocess.run([drv, what], check=True, capture_output=True, text=True, input="\n".join(lines) + "\n").stdout.splitlines()


# ---------------------------------------------------------------- the rules header against the reference
def test_priority_and_keys(driver):
    top = 2 ** 32 - 1
    lens = [0, 1, 2, top - 1, top]
    idx = [0, 1, 2, 7, 0xFFFFFFEF, top - 1]
    cases = [(lu, u, lv, v) for lu in lens for lv in lens for u in idx for v in idx if u != v]
    out = run(driver, "before", ["%d %d %d %d" % c for c in cases])
    assert len(out) == len(cases)
    for (lu, u, lv, v), line in zip(cases, out):
        buv, bvu, ku, kv, back = [int(x) for x in line.split()]
        assert bool(buv) == R.before(lu, u, lv, v) and bool(bvu) == R.before(lv, v, lu, u)
        assert buv + bvu == 1                                      # a total order on distinct nodes
        assert ku == R.key(lu, u) and kv == R.key(lv, v) and back == u == R.key_index(ku)
        assert (ku > kv) == bool(buv)                              # an integer max picks the first in priority order


def test_node_predicate(driver):
    n = 24
    blocks = [(0, n, 0, n, 1), (3, 9, 3, 9, 1), (0, 1, 0, 1, 1),                       # upper: one range
              (5, 10, 20, 4, 0), (2, 5, 7, 6, 0), (2, 8, 6, 9, 0), (4, 12, 6, 3, 0),     # a gap, touching, overlapping, nested
              (10, 6, 0, 4, 0), (0, 1, 1, 23, 0), (7, 1, 7, 1, 0), (0, n, 0, n, 0)]
    out = run(driver, "nodes", ["%d %d %d %d %d %d" % (b + (n,)) for b in blocks])
    for (qf, qc, tf, tc, up), line in zip(blocks, out):
        got = [int(x) for x in line.split()]
        want = [int(R.is_node(v, qf, qc, tf, tc)) for v in range(n)]
        assert got[1:] == want
        assert got[0] == sum(want) == R.node_count(qf, qc, tf, tc)
    out = run(driver, "all", ["0", "1", "5"])
    assert [[int(x) for x in line.split()] for line in out] == [[0, 0, 0, 0], [1, 1, 0, 0, 0], [5, 1, 1, 1, 1, 1, 0, 0, 0]]


# ---------------------------------------------------------------- the reference against a breadth-first restatement
def bfs_components(n, a, b):
    adj = [set() for _ in range(n)]
    for u, v in zip(a, b):
        adj[u].add(v)
        adj[v].add(u)
    label = [None] * n
    for s in range(n):                        # ascending: the first node to reach a component is its smallest
        if label[s] is None:
            todo = [s]
            label[s] = s
            while todo:
                x = todo.pop(0)
                for y in adj[x]:
                    if label[y] is None:
                        label[y] = s
                        todo.append(y)
    return label


def slow_greedy(n, a, b, lengths):
    ln = [0] * n if lengths is None else lengths
    order = sorted(range(n), key=lambda v: (-ln[v], v))
    reps, label = [], [None] * n
    for v in order:
        mine = [r for r in reps if any((u == r and w == v) or (u == v and w == r) for u, w in zip(a, b))]
        label[v] = mine[0] if mine else v
        if not mine:
            reps.append(v)
    return label


def check_reference(n, a, b, lengths):
    want_c = bfs_components(n, a, b)
    lab, recs, summ, mem = R.cluster(R.COMPONENTS, n, a, b, lengths)
    assert lab == want_c
    lab_g, recs_g, summ_g, mem_g = R.cluster(R.GREEDY, n, a, b, lengths)
    assert lab_g == slow_greedy(n, a, b, lengths)
    ln = [0] * n if lengths is None else lengths
    for labels, rr, ss, mm in ((lab, recs, summ, mem), (lab_g, recs_g, summ_g, mem_g)):
        assert [r[0] for r in rr] == sorted(set(labels)) and sum(r[1] for r in rr) == n == ss["nodes"]
        assert [r[0] for r in rr] == [m[0] if labels is lab else r[0] for r, m in zip(rr, mm)]
        for (l, size, longest, edges), m in zip(rr, mm):
            assert m == [v for v in range(n) if labels[v] == l] and size == len(m)
            assert longest == max(m, key=lambda v: R.key(ln[v], v))
            assert edges == sum(1 for u, v in zip(a, b) if u != v and labels[u] == l and labels[v] == l)
        assert ss["clusters"] == len(rr) and ss["singletons"] == sum(1 for r in rr if r[1] == 1)
        assert ss["self_edges"] == sum(1 for u, v in zip(a, b) if u == v) and ss["edges"] + ss["self_edges"] == len(a)
    assert all(r[2] == r[0] for r in recs_g)                      # greedy: the representative is the cluster's first
    assert summ["edges"] == sum(r[3] for r in recs)               # components: every real edge lies within a cluster


def test_reference_on_every_small_graph():
    rng = random.Random(5)
    for n in range(0, 6):
        pairs = list(itertools.combinations(range(n), 2))
        for mask in range(1 << len(pairs)):
            a = [p[0] for k, p in enumerate(pairs) if mask >> k & 1]
            b = [p[1] for k, p in enumerate(pairs) if mask >> k & 1]
            check_reference(n, a, b, None)
            check_reference(n, b, a, [rng.randrange(3) for _ in range(n)])


def test_reference_on_random_graphs():
    rng = random.Random(11)
    for _ in range(300):
        n = rng.randrange(1, 31)
        m = rng.randrange(0, 50)
        a = [rng.randrange(n) for _ in range(m)]
        b = [rng.randrange(n) for _ in range(m)]              # self edges and duplicates happen
        check_reference(n, a, b, [rng.randrange(4) for _ in range(n)] if rng.random() < 0.7 else None)


# ---------------------------------------------------------------- the companion header and its mirrors
def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared(path):
    return sorted(set(re.findall(r"\b(aln_[a-z_0-9]+)\s*\(", strip_comments(open(path).read()))))


def test_the_companion_header_declares_the_cluster_exports():
    assert declared(os.path.join(ROOT, "include", "aligner_hip_cluster.h")) == sorted(_ffi.CLUSTER_EXPORTS)
    assert len(declared(os.path.join(ROOT, "include", "aligner_hip.h"))) == 61         # the main header is as it was
    assert not set(_ffi.CLUSTER_EXPORTS) & set(_ffi.EXPORTS)
    assert "aln_cluster.hip" in native_build.SOURCES and "aln_cluster_rules.h" in native_build.HEADERS


def test_the_library_exports_them_with_argtypes():
    native_build.build()
    lib = _ffi.load()
    for sym in _ffi.CLUSTER_EXPORTS:
        fn = getattr(lib, sym)
        assert fn.argtypes is not None and fn.restype is C.c_int, sym
    assert lib.aln_abi_version() == 2


def test_every_export_is_called_from_c99():
    src = strip_comments(open(os.path.join(ROOT, "tests", "abi_cluster.c")).read())
    for sym in _ffi.CLUSTER_EXPORTS:
        assert re.search(r"\b%s\s*\(" % sym, src), sym


def test_the_header_compiles_as_c99_and_the_layouts_match(tmp_path):
    native_build.build()
    src = str(tmp_path / "only.c")
    with open(src, "w") as fh:
        fh.write('#include "aligner_hip_cluster.h"\nint main(void) { return (int)sizeof(aln_cluster_record) - 16; }\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                           str(tmp_path / "only.o")])
    exe = native_build.build_cluster_harness()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("layout ")]
    assert [l[1] for l in lines] == ["aln_cluster_record", "aln_cluster_summary"]
    for l, cls in zip(lines, (_ffi.ClusterRecord, _ffi.ClusterSummary)):
        assert int(l[2]) == C.sizeof(cls)
        fields = [(l[k], int(l[k + 1]), int(l[k + 2])) for k in range(3, len(l), 3)]
        assert fields == [(name, getattr(cls, name).offset, getattr(cls, name).size) for name, _t in cls._fields_]
    assert C.sizeof(_ffi.ClusterRecord) == 16 and C.sizeof(_ffi.ClusterSummary) == 48
    from aligner_amd import cluster
    assert cluster.RECORD_DTYPE.itemsize == 16 and list(cluster.RECORD_DTYPE.names) == [f[0] for f in _ffi.ClusterRecord._fields_]
    assert cluster.NONE == R.NONE == 0xFFFFFFFF and cluster.MODES == {"components": R.COMPONENTS, "greedy": R.GREEDY}


# ---------------------------------------------------------------- refusals that need no device
def test_refusals_without_a_device():
    native_build.build()
    lib = _ffi.load()
    INV = _ffi.ERR_INVALID_ARGUMENT
    label = (C.c_uint32 * 4)(7, 7, 7, 7)
    a, b = (C.c_uint32 * 2)(0, 1), (C.c_uint32 * 2)(1, 2)
    summ = _ffi.ClusterSummary(9, 9, 9, 9, 9, 9, 9)

    def untouched():
        return list(label) == [7, 7, 7, 7] and (summ.nodes, summ.clusters, summ.edges, summ.self_edges, summ.singletons, summ.rounds, summ.reserved) == (9,) * 7

    # a null context; an unknown mode (refused before anything else is looked at)
    assert lib.aln_cluster_edges(None, 0, 4, None, a, b, 2, label, None, 0, C.byref(summ)) == INV and untouched()
    assert lib.aln_cluster_edges(None, 2, 4, None, a, b, 2, label, None, 0, C.byref(summ)) == INV and b"mode" in lib.aln_last_error() and untouched()
    assert lib.aln_cluster_edges(None, 0xFFFFFFFF, 0, None, None, None, 0, None, None, 0, C.byref(summ)) == INV and untouched()
    assert lib.aln_cluster_edges(None, 1, 4, None, a, b, 2, label, None, 0, None) == INV and untouched()
    # a null set
    assert lib.aln_seqset_held_cluster(None, None, 0, None, 0, label, None, 0, C.byref(summ)) == INV and untouched()
    assert lib.aln_seqset_held_cluster(None, None, 0, None, 5, label, None, 0, None) == INV and untouched()
    from aligner_amd import cluster
    with pytest.raises(ValueError):
        cluster.mode_code("average")
    with pytest.raises(ValueError):
        cluster.cluster_edges(3, [0, 1], [1], mode="components")
