"""Heuristic alignment of the pairs of a sequence set, as far as it can be checked without a GPU: aln_loop_rules.h compiled for the host
against a Python restatement, the numbering of every window of a block (the host walk of aln_pairset_create_from_set and the numpy
form PairSet.from_seqset uses) against tests/seqset_ref.py, the exported symbols, and heuristic.align_set's driver on an oracle-backed
stand-in for the derived pair set."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import seqset_ref  # noqa: E402
import set_loop_cases as cases  # noqa: E402

from aligner_amd import _ffi  # noqa: E402
from aligner_amd.enums import Protein  # noqa: E402
from aligner_amd.errors import AlignerError, ErrorKind, ReferencePanic  # noqa: E402
from aligner_amd.heuristic import align_set  # noqa: E402  (the feature: absent on the parent commit)
from aligner_amd.simple import Heuristics  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aligner_amd", "csrc")
NEW = ["aln_pairset_create_from_set", "aln_pairset_loop_begin", "aln_pairset_loop_step"]

RULES = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "aln_loop_rules.h"
static double bits(const char *s) { unsigned long long u = strtoull(s, 0, 16); double d; memcpy(&d, &u, 8); return d; }
int main(int argc, char **argv)
{
    // <status> <f bits> <best bits> ... -> per triple "class finished after_ok after_noroot"
    for (int i = 1; i + 2 < argc; i += 3) {
        const uint32_t c = aln_loop_classify((int32_t)atoi(argv[i]), bits(argv[i + 1]), bits(argv[i + 2]));
        printf("%u %d %u %u\n", c, aln_loop_is_finished(c) ? 1 : 0, aln_loop_after_transform(0), aln_loop_after_transform(ALN_TRANSFORM_NO_ROOT));
    }
    return 0;
}
"""

WINDOW = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "aln_seqset_rules.h"
int main(int argc, char **argv)
{
    // <n_seqs> <q_first> <q_count> <t_first> <t_count> <upper>: every window (first, n) of the block, one line each: "first n q t q t .."
    if (argc < 7) return 2;
    aln_seqset_block b;
    const uint64_t n_seqs = strtoull(argv[1], 0, 10);
    b.q_first = strtoull(argv[2], 0, 10); b.q_count = strtoull(argv[3], 0, 10); b.t_first = strtoull(argv[4], 0, 10); b.t_count = strtoull(argv[5], 0, 10);
    b.upper = (uint32_t)strtoul(argv[6], 0, 10); b.reserved = 0;
    const uint64_t pairs = aln_seqset_block_pairs(n_seqs, b);
    std::vector<uint64_t> q(pairs + 2, 777), t(pairs + 2, 777);
    for (uint64_t first = 0; first <= pairs; ++first)
        for (uint64_t n = 0; first + n <= pairs; ++n) {
            aln_seqset_window(b, first, n, q.data(), t.data());
            if (q[n] != 777 || t[n] != 777) return 3;               // nothing beyond the window
            printf("%llu %llu", (unsigned long long)first, (unsigned long long)n);
            for (uint64_t i = 0; i < n; ++i) printf(" %llu %llu", (unsigned long long)q[i], (unsigned long long)t[i]);
            printf("\n");
            for (uint64_t i = 0; i < n; ++i) q[i] = t[i] = 777;
        }
    return 0;
}
"""


def _compile(tmp, name, src):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    path = os.path.join(str(tmp), name + ".cpp")
    with open(path, "w") as fh:
        fh.write(src)
    exe = os.path.join(str(tmp), name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, path, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def lib():
    from aligner_amd import build as native_build
    native_build.build()
    return _ffi.load()


def _hex(x):
    return "%016x" % np.array([x], dtype=np.float64).view(np.uint64)[0]


def test_loop_rules_header_against_a_restatement(tmp_path):
    exe = _compile(tmp_path, "rules", RULES)
    inf, nan = math.inf, math.nan
    values = [0.0, -0.0, 1.0, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, 5e-324, -5e-324, 37.25, -3.0, inf, -inf, nan, -nan]
    triples = [(0, f, b) for f in values for b in values]
    # f above, equal to and below best are all there, and +0.0 against -0.0 both ways
    assert (0, 1.0 + 2.0 ** -52, 1.0) in triples and (0, 1.0, 1.0) in triples and (0, 1.0 - 2.0 ** -53, 1.0) in triples
    triples += [(st, f, b) for st in range(1, 11) for f, b in ((1.0, 0.0), (0.0, 1.0), (nan, nan), (inf, 0.0))]          # every failure status
    triples += [(-1, 1.0, 0.0)]
    args = [x for st, f, b in triples for x in (str(st), _hex(f), _hex(b))]
    out = subprocess.check_output([exe] + args, text=True).split("\n")[:-1]
    assert len(out) == len(triples)
    seen = set()
    for (st, f, b), line in zip(triples, out):
        c, fin, ok, noroot = (int(x) for x in line.split())
        want = cases.classify(st, f, b)
        assert c == want and fin == (1 if want <= 2 else 0), (st, f, b, line)
        assert ok == 4 and noroot == cases.NO_ROOT
        seen.add(c)
    assert seen == {0, 1, 3}
    # the restatement itself on the cases that matter
    assert cases.classify(0, 0.0, -0.0) == 0 and cases.classify(0, -0.0, 0.0) == 0 and cases.classify(0, nan, 0.0) == 0
    assert cases.classify(0, 1.0, nan) == 0 and cases.classify(0, inf, 1e308) == 3 and cases.classify(0, inf, inf) == 0
    assert cases.classify(0, 0.0, -inf) == 3 and cases.classify(3, inf, 0.0) == 1
    assert (_ffi.LOOP_CAUSE_DONE, _ffi.LOOP_CAUSE_FAILED, _ffi.LOOP_CAUSE_NO_ROOT) == (cases.DONE, cases.FAILED, cases.NO_ROOT)


BLOCKS = [(9, (0, 9, 0, 9, 1)), (12, (3, 7, 3, 7, 1)), (5, (0, 2, 0, 2, 1)), (10, (1, 4, 2, 8, 0)), (7, (0, 7, 6, 1, 0)), (6, (5, 1, 0, 6, 0)),
          (9, (0, 5, 0, 5, 0))]


def test_every_window_of_a_block_is_numbered_as_the_reference_list(tmp_path):
    from aligner_amd.seqset import window
    exe = _compile(tmp_path, "window", WINDOW)
    inside = 0
    for n_seqs, b in BLOCKS:
        ref = cases.block_list(n_seqs, b)
        assert len(ref) <= 40
        lines = subprocess.check_output([exe, str(n_seqs)] + [str(x) for x in b], text=True).split("\n")[:-1]
        assert len(lines) == (len(ref) + 1) * (len(ref) + 2) // 2
        blk = _ffi.SeqsetBlock(b[0], b[1], b[2], b[3], b[4], 0)
        for line in lines:
            w = [int(x) for x in line.split()]
            first, n = w[0], w[1]
            got = list(zip(w[2::2], w[3::2]))
            assert got == ref[first:first + n], (b, first, n)
            q, t = window(blk, first, n)                             # the numpy form
            assert list(zip(q.tolist(), t.tolist())) == got, (b, first, n)
            if b[4] and n and got[0][1] != got[0][0] + 1 and got[-1][1] != b[0] + b[1] - 1:
                inside += 1                                          # starts and ends inside a row of the triangle
    assert inside > 100


def test_library_exports_the_new_symbols(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aligner_hip.h")).read(), flags=re.S)
    for sym in NEW:
        assert sym in _ffi.EXPORTS and hasattr(lib, sym), sym
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % sym, hdr)
        assert decl, sym
        assert len(getattr(lib, sym).argtypes) == len([a for a in decl.group(1).split(",") if a.strip()]), sym
    assert lib.aln_abi_version() == 2
    rust = open(os.path.join(ROOT, "rust", "aligner-core-hip", "src", "lib.rs")).read()
    assert all("fn %s(" % sym in rust for sym in NEW)


def test_argument_validation_without_a_device(lib):
    st = C.c_int(-1)
    blk = _ffi.SeqsetBlock(0, 2, 0, 2, 1, 0)
    assert not lib.aln_pairset_create_from_set(None, C.byref(blk), 0, 1, C.byref(st)) and st.value == _ffi.ERR_INVALID_ARGUMENT
    m, s4 = np.zeros(16), np.zeros(4, np.int32)
    assert lib.aln_pairset_loop_begin(None, m.ctypes.data, s4.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    p = _ffi.Params(_ffi.CORE_LOCAL, 0, 11.0, 2.0, None, 24, 24, 24, 0, 98, 0, 0, 0, 0)
    assert lib.aln_pairset_loop_step(None, None, None, None, None, None) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_pairset_loop_step(None, C.byref(p), None, None, None, None) == _ffi.ERR_INVALID_ARGUMENT
    for sem in (_ffi.LEGACY_GLOBAL, _ffi.LEGACY_LOCAL, _ffi.PWM_LOCAL):
        p.semantics = sem
        assert lib.aln_pairset_loop_step(None, C.byref(p), None, None, None, None) == _ffi.ERR_UNSUPPORTED


# ---------------------------------------------------------------- the driver
def _set(n=7, seed=12):
    from test_pairset_cpu import recipe_pairs
    pairs, _ = recipe_pairs(n, seed, lo=40, hi=120)
    seqs = [q for q, _ in pairs]
    for i in range(1, n):
        L = min(len(seqs[i]), len(seqs[i - 1]), 30)
        seqs[i][:L] = seqs[i - 1][-L:]
    return seqs


def _check(orc, seqs, got, qt, heur, matrix, del_, ext, first=0):
    assert [(g[0], g[1], g[2]) for g in got] == [(first + k, q, t) for k, (q, t) in enumerate(qt)]
    kinds = set()
    for (k, q, t, r) in got:
        h = heur(q, t) if callable(heur) else heur
        r2 = h.r_squared if abs(h.r_squared) >= np.finfo(np.float64).eps else 576.0
        want = cases.replay(orc, seqs[q], seqs[t], matrix, h.kd, r2, h.frequencies, del_, ext, 24)
        if want["begin"] or want["cause"] == cases.NO_ROOT:
            assert isinstance(r, ReferencePanic) and r.status == -1, (q, t)
            kinds.add("no-root")
        elif want["cause"] == cases.FAILED:
            assert isinstance(r, ReferencePanic) and r.status == want["status"], (q, t)
            kinds.add(want["status"])
        else:
            ref = want["ref"]
            assert r.alignment.f == ref["f"] and r.alignment.coords == ref["coords"] and r.score == ref["score"], (q, t)
            assert r.alignment.query.tolist() == ref["qa"].tolist() and r.alignment.target.tolist() == ref["ta"].tolist(), (q, t)
            assert r.matrix.tobytes() == np.ascontiguousarray(want["matrix"]).tobytes(), (q, t)
            kinds.add("ok%d" % want["step"])
    return kinds


def test_align_set_driver_on_an_oracle_backend(orc, blosum62):
    seqs = _set()
    seqs[3] = np.zeros(0, np.uint8)                                                          # an empty sequence
    seqs[5] = np.concatenate([seqs[5][:10], np.array([30], np.uint8)])                       # a code outside the matrix
    ss = cases.FakeSeqSet(seqs, Protein)

    def heur(q, t):
        fr = np.bincount(np.minimum(seqs[t], 23), minlength=24).astype(np.float64) / max(len(seqs[t]), 1)
        r2 = 1e-9 if (q, t) == (0, 2) else (0.0 if (q + t) % 2 else 576.0)                   # no root; 0 -> rows * cols
        return Heuristics(kd=[-0.2, -0.5, -1.0][(q + t) % 3], r_squared=r2, frequencies=fr)

    qt = cases.block_list(7, (0, 7, 0, 7, 1))
    cases.OracleSetLoop.made = []
    got = list(align_set(ss, 11.0, 2.0, blosum62, heur, max_pairs=8, backend=cases.OracleSetLoop))
    made = cases.OracleSetLoop.made
    assert [(m.first, m.n) for m in made] == [(0, 8), (8, 8), (16, 5)] and all(m.closed for m in made)      # the slice cuts
    kinds = _check(orc, seqs, got, qt, heur, blosum62, 11.0, 2.0)
    assert {"no-root", _ffi.ERR_EMPTY_SEQUENCE, _ffi.ERR_CODE_OUT_OF_RANGE} <= kinds and len([k for k in kinds if str(k).startswith("ok")]) >= 2, kinds
    # one slice gives the same, a rectangle, one Heuristics for all, and errors="raise"
    one = list(align_set(ss, 11.0, 2.0, blosum62, heur, backend=cases.OracleSetLoop))
    assert len(one) == 21 and all(type(a[3]) is type(b[3]) for a, b in zip(one, got))
    assert all(isinstance(a[3], Exception) or a[3].matrix.tobytes() == b[3].matrix.tobytes() for a, b in zip(one, got))
    h1 = Heuristics(kd=-0.5, r_squared=0.0, frequencies=np.full(24, 1.0 / 24))
    rect = (0, 2, 4, 3, 0)
    got = list(align_set(ss, 8.0, 8.0, blosum62, h1, block=rect, max_pairs=4, backend=cases.OracleSetLoop))
    _check(orc, seqs, got, cases.block_list(7, rect), h1, blosum62, 8.0, 8.0)
    with pytest.raises(ReferencePanic) as e:
        list(align_set(ss, 11.0, 2.0, blosum62, heur, errors="raise", backend=cases.OracleSetLoop))
    assert e.value.status == -1                                                              # pair (0, 2) comes first in pair order
    # the panic is raised when its pair is reached: pair 0 is yielded before it
    it = align_set(ss, 11.0, 2.0, blosum62, heur, errors="raise", backend=cases.OracleSetLoop)
    assert next(it)[0] == 0


def test_align_set_argument_errors(blosum62):
    ss = cases.FakeSeqSet(_set(4), Protein)
    h = Heuristics(kd=-0.5, r_squared=576.0, frequencies=np.full(24, 1.0 / 24))
    with pytest.raises(AlignerError) as e:
        list(align_set(ss, 11.0, 2.0, blosum62, None, backend=cases.OracleSetLoop))
    assert e.value.kind == ErrorKind.MissingArgument
    for kw in (dict(errors="ignore"), dict(max_pairs=0), dict(block=(0, 5, 0, 5, 1)), dict(block=(0, 4, 1, 3, 1))):
        with pytest.raises(ValueError):
            list(align_set(ss, 11.0, 2.0, blosum62, h, backend=cases.OracleSetLoop, **kw))
    with pytest.raises(ValueError):
        list(align_set(ss, 11.0, 2.0, blosum62[:20, :20], h, backend=cases.OracleSetLoop))
