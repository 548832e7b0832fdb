"""Block-to-quad placement of the direction words (FastStrip::block / quad, aln_fast.h): a quad's four blocks are four constant
components of one 16-byte store, so what can go wrong is a block's word landing in another component, a last quad that ends
after 1, 2, 3 or 4 blocks, and a strip whose rows-per-lane count R takes another block length.

Every pair goes through aln_align_pair on the batch fast kernel (ALN_NO_SINGLE=1; flags say which kernel filled it) and is compared
with the CPU oracle: summary, both strings and the whole direction matrix D.

* step counts, R = 8 (M = 512): N = 65..72 and 129..136 -- N + 63 steps takes every residue mod 8, so the last quad ends after
  1, 2, 3 or 4 blocks of two steps, with and without a half block;
* rows: M in {8, 64, 65, 511, 512, 513, 576, 1030} -- one strip at R = 1, 2 and 8, a full strip plus an R = 1, 2 or 8
  remainder, three strips;
* every R in 1..8: M = 64 R - 1, N = 70;
* strip 0's form with the advice feed and the repair run: a catalogue pair of advice_model.py whose advice flips (its own scoring
  scheme, as test_row1_repair_gpu.py builds it); its route must be the parent's;
* core global, 150 x 150, +5 / -4, 10 / 1: the shared header still serves it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import advice_model as am  # noqa: E402
from aligner_amd import _ffi, runtime  # noqa: E402
from aligner_amd.matrices import get_blosum62  # noqa: E402

pytestmark = pytest.mark.gpu

_refs = {}


def pair(M, N):
    """(q, t): N query and M target residues, seeded by the shape; t carries a mutated copy of a piece of q so that the local
    alignment is not trivial."""
    rng = np.random.RandomState(1000 * M + N)
    q = rng.randint(0, 20, size=N).astype(np.uint8)
    t = rng.randint(0, 20, size=M).astype(np.uint8)
    n = min(M, N) // 2
    if n >= 4:
        piece = q[N - n:].copy()
        piece[::5] = rng.randint(0, 20, size=len(piece[::5]))
        t[M - n:] = piece
    return q, t


def reference(orc, sem, M, N, S, de, ex):
    """The oracle's result for the pair, computed once and left unchanged."""
    key = (sem, M, N, de, ex)
    if key not in _refs:
        q, t = pair(M, N)
        ref = orc.align(sem, q, t, de, ex, S, want_matrices=True)
        assert ref["status"] == 0
        _refs[key] = (q, t, ref)
    return _refs[key]


def check(res, qa, ta, D, ref, where):
    assert res.status == 0, where
    assert (res.score, res.f) == (ref["score"], ref["f"]), where
    assert (res.end_y, res.end_x) == ref["end"], where + ((res.end_y, res.end_x), ref["end"])
    assert (res.start_y, res.start_x) == ref["start"], where
    assert res.aln_len == len(ref["qa"]) and qa.tolist() == ref["qa"].tolist() and ta.tolist() == ref["ta"].tolist(), where
    bad = np.argwhere(D != ref["D"])
    assert len(bad) == 0, where + ("D differs in %d cells, first at (y, x) = %s" % (len(bad), bad[0]),)


def run_local(orc, monkeypatch, M, N):
    S = get_blosum62()
    q, t, ref = reference(orc, orc.CORE_LOCAL, M, N, S, 11, 2)
    monkeypatch.setenv("ALN_NO_SINGLE", "1")
    res, qa, ta, D, _ = runtime.align_pair(_ffi.CORE_LOCAL, q, t, 11, 2, S, want_directions=True)
    where = ("M", M, "N", N, hex(res.passes))
    assert (res.flags & 0xe) == 8, where + (res.flags,)          # the batch fast kernel
    check(res, qa, ta, D, ref, where)


@pytest.mark.parametrize("N", list(range(65, 73)) + list(range(129, 137)))
def test_last_quad_ends_after_every_block_count(orc, monkeypatch, N):
    run_local(orc, monkeypatch, 512, N)


@pytest.mark.parametrize("M", [8, 64, 65, 511, 512, 513, 576, 1030])
def test_rows(orc, monkeypatch, M):
    run_local(orc, monkeypatch, M, 70)


@pytest.mark.parametrize("R", range(1, 9))
def test_every_rows_per_lane_count(orc, monkeypatch, R):
    run_local(orc, monkeypatch, 64 * R - 1, 70)


# The route of the hazard pair below (full passes, repair rounds, checkpoint slot, escalation reason).  Not recorded from a run of
# the parent made for this test: it is the catalogue line's own route in advice_model.py, which tests/test_row1_repair_gpu.py
# asserts on the GPU and which the parent's kernel passed there -- the parent's value by that test, not by a measurement here.
HAZARD_PAIR = "h256_128"
HAZARD_ROUTE_PARENT = dict(full=1, repairs=1, slot=4, reason=0)


def test_strip0_with_advice_and_repair(orc, monkeypatch):
    entry = [e for e in am.CATALOGUE if e[0] == HAZARD_PAIR][0]
    q, t, S, de, ex = am.entry_pair(entry)
    ref = orc.align(orc.CORE_LOCAL, q, t, de, ex, S, want_matrices=True)
    monkeypatch.setenv("ALN_NO_SINGLE", "1")
    res, qa, ta, D, _ = runtime.align_pair(_ffi.CORE_LOCAL, q, t, de, ex, S, want_directions=True)
    where = (HAZARD_PAIR, hex(res.passes))
    assert (res.flags & 0xe) == 8, where + (res.flags,)
    check(res, qa, ta, D, ref, where)
    got = am.decode_passes(res.passes)
    assert {k: got[k] for k in HAZARD_ROUTE_PARENT} == HAZARD_ROUTE_PARENT, where + (got,)


def test_core_global(orc, monkeypatch):
    B = get_blosum62()
    S = np.where(np.eye(B.shape[0], dtype=bool), 5, -4).astype(B.dtype)
    q, t, ref = reference(orc, orc.CORE_GLOBAL, 150, 150, S, 10, 1)
    monkeypatch.setenv("ALN_NO_SINGLE", "1")
    res, qa, ta, D, _ = runtime.align_pair(_ffi.CORE_GLOBAL, q, t, 10, 1, S, want_directions=True)
    assert (res.flags & 0xe) == 8, ("global 150 x 150", res.flags)          # the batch fast kernel
    check(res, qa, ta, D, ref, ("global 150 x 150",))
