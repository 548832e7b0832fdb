"""The CPU model of the row-1 speculation (advice_model.py) is right, and its catalogue is what it claims to be.
* Iterating b := z until the advice is self-consistent gives exactly the oracle's H on seeded small pairs (del < ext included);
  pyref.core agrees on the smallest; the anti-diagonal fill equals the literal column-major loop nest under arbitrary advice.
* Every catalogue line falls into its declared class under classify, and predict gives its declared route -- certified here, on
  the CPU, so that tests/test_row1_repair_gpu.py cannot lose coverage because an input drifted.
* checkpoint_steps and the geometry helpers against values written out by hand."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import advice_model as am  # noqa: E402
import pyref  # noqa: E402

SMALL = [(5, 9, (2, 1)), (7, 50, (1, 2)), (40, 300, (2, 1)), (64, 200, (11, 2)), (100, 130, (3, 1)), (130, 90, (1, 3))]


@pytest.mark.parametrize("M,N,gaps", SMALL)
def test_fixed_point_of_the_model_is_the_oracles_matrix(orc, M, N, gaps):
    S = am.pm1_scheme()
    for seed in range(4):
        q, t = am.random_pair(M, N, 100 * seed + M)
        H, fills = am.fixed_point(q, t, S, *gaps)
        ref = orc.align(orc.CORE_LOCAL, q, t, gaps[0], gaps[1], S, want_matrices=True)
        assert ref["status"] == 0
        assert np.array_equal(H, ref["H"]), (M, N, gaps, seed)
        if M * N <= 400:
            py = pyref.core(q.tolist(), t.tolist(), gaps[0], gaps[1], S.tolist(), True)
            assert all(py["H"][(y, x)] == H[y, x] for y in range(M + 1) for x in range(N + 1))


def test_wavefront_fill_equals_the_column_major_loop_nest():
    rng = np.random.default_rng(5)
    for M, N, gaps, S in ((9, 40, (2, 1), am.pm1_scheme()), (33, 70, (1, 2), am.pm1_scheme()), (20, 60, (3, 1), am.planted_scheme())):
        q, t = am.random_pair(M, N, M)
        for _ in range(3):
            b = rng.integers(0, 2, N + 2).astype(bool)
            assert np.array_equal(am.spec_fill(q, t, S, gaps[0], gaps[1], b), am.spec_fill_colmajor(q, t, S, gaps[0], gaps[1], b))


def test_checkpoint_steps_by_hand():
    want = {1: [64, 128, 256, 512, 1024], 2: [32, 64, 128, 256, 512, 1024]}
    for R in range(3, 9):
        want[R] = [16, 32, 64, 128, 256, 512, 1024]
    for R in range(1, 9):
        assert am.checkpoint_steps(R) == want[R], R
        assert am.checkpoint_steps(R, 512) == want[R][:-1], R
    assert [am.spb(R) for R in range(1, 9)] == [16, 8, 4, 4, 2, 2, 2, 2]
    assert [am.pick_r(M) for M in (1, 64, 65, 128, 192, 256, 320, 384, 448, 449, 512)] == [1, 1, 2, 2, 3, 4, 5, 6, 7, 8, 8]
    g = am.Geometry(600, 1300)
    assert (g.ns, g.R, g.rows, g.lanes, g.nsteps, g.total) == (2, 8, 512, 64, 1363, 1368)
    g = am.Geometry(40, 300)
    assert (g.ns, g.R, g.lanes, g.nsteps, g.total, g.fill_rows) == (1, 1, 40, 339, 384, 64)


def test_decode_passes():
    assert am.decode_passes(0x00070101) == dict(full=1, fallback=False, repairs=1, slot=7, reason=0)
    assert am.decode_passes(0x00300183) == dict(full=3, fallback=True, repairs=1, slot=0, reason=3)
    assert am.decode_passes(0x00140202) == dict(full=2, fallback=False, repairs=2, slot=4, reason=1)


@pytest.fixture(scope="module")
def certified():
    out = {}
    for e in am.CATALOGUE:
        q, t, S, de, ex = am.entry_pair(e)
        out[e[0]] = (am.classify(q, t, S, de, ex), am.predict(q, t, S, de, ex), am.Geometry(len(t), len(q)))
    return out


@pytest.mark.parametrize("entry", am.CATALOGUE, ids=[e[0] for e in am.CATALOGUE])
def test_catalogue_entry_is_in_its_class(certified, entry):
    name, cls, _, _, _, _, route = entry
    c, p, g = certified[name]
    assert (p["full"], p["repairs"], p["slot"], p["reason"]) == route
    assert p["exact_stale"] and not p["fallback"]
    steps = am.checkpoint_steps(g.R)
    if cls == "consistent":
        assert c["consistent"] and c["last_flip"] == 0
        return
    assert not c["consistent"]
    if cls == "harmless":
        assert c["cells"] == 0 and c["consistent_after"] and c["last_flip"] <= am.CK_LAST
        slot = next(i for i, s in enumerate(steps) if s >= c["last_flip"])
        assert steps[slot] < g.total                   # the strip does reach that checkpoint
        assert route == (1, 1, slot + 1, 0)
    elif cls == "dies_out":
        assert c["cells"] > 0 and c["consistent_after"] and not c["bottom_row_differs"]
        assert c["last_step"] < p["ck_step"] - 2 and c["last_flip"] <= p["ck_step"] and route[3] == 0
    elif cls == "beyond":
        assert c["last_flip"] > am.CK_LAST and route == (2, 1, 0, 1)
    elif cls == "bottom_row":
        assert g.ns > 1 and c["bottom_row_differs"] and route[0] >= 2 and route[3] != 0
    elif cls == "no_rejoin":
        assert c["last_flip"] <= 512 and c["last_step"] >= 512 and g.total > 1024 and route[3] == 3
        assert c["last_step"] < 1022                   # the checkpoint at 1024 would have matched: the rule at 512 is what stops it
    elif cls == "unsettled":
        assert g.ns == 1 and not c["consistent_after"] and route[0] >= 3
    elif cls == "rounds":
        assert g.ns == 1 and not c["consistent_after"] and route[1] >= 2 and route[3] == 0
        H, _ = am.fixed_point(*am.entry_pair(entry))
        assert np.array_equal(p["H"], H) and p["end"] == am._argmax(H)     # re-run prefixes over one another: still the reference's fill
    elif cls == "stale":
        assert p.get("stale") and c["end0"] != c["end1"] and c["last_step"] < 1022 and route == (2, 1, 0, 3)
    else:
        raise AssertionError(cls)


def test_catalogue_covers_every_slot_reason_and_variant(certified):
    routes = {e[0]: e[6] for e in am.CATALOGUE}
    ok = [n for n, r in routes.items() if r[3] == 0 and r[1] >= 1]
    assert {routes[n][2] for n in ok} == set(range(1, 8))
    assert {r[3] for r in routes.values()} >= {1, 2, 3}
    assert any(certified[n][2].ns == 1 for n in ok) and any(certified[n][2].ns > 1 for n in ok)
    assert {certified[n][2].R for n in ok if certified[n][2].ns == 1} == set(range(1, 9))       # every R of aln_pick_r
    # last_flip exactly on a checkpoint step and one behind it (the `<=` of "in.last_flip <= next_ck")
    flips = {certified[n][0]["last_flip"] for n in ok}
    assert {16, 17, 32, 33, 64, 128, 129, 256, 257, 512, 513, 1024} <= flips
    # the entries of (512, 1024] escalate with reason 1 when the last checkpoint is 512
    late = [e for e in am.CATALOGUE if 512 < certified[e[0]][0]["last_flip"] <= 1024]
    assert len(late) >= 4 and any(certified[e[0]][0]["cells"] for e in late)
    for e in late:
        p = am.predict(*am.entry_pair(e), ck_last=512)
        assert (p["full"], p["repairs"], p["slot"], p["reason"]) == (2, 1, 0, 1), e[0]
    assert 30 <= len(am.CATALOGUE) <= 40
