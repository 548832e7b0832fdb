"""The CPU model of the generic kernels' row-1 advice passes (advice_generic_model.py) is right, its catalogue is what it claims
to be, and the catalogue can see the defects it was built for.
* Whenever the model converges, the last pass's H, every direction tag (row 1 among them) and the zero row are the oracle's;
  the lines that end in the strict-order routine are iterated on to their fixed point and compared there.
* Every catalogue line has its declared outcome, pass count and properties (what forced the second pass, the one deciding
  column, a tag decided inside f64::EPSILON) -- from the oracle and the model alone, so that tests/test_advice_generic_gpu.py
  cannot lose coverage because an input drifted.  A pass accepted as "same" is re-filled under its own zeros and compared cell
  for cell (inside predict_generic): the induction adopt_advice_checked rests on, executed.
* max_passes 1..3: the strict-order routine exactly when the model needs more.
* Planted defects, in the style of test_tb_batch_model_cpu.py: each wrong rule gives a wrong passes word, or a matrix that is
  not the oracle's, on a named line.  One listed defect cannot be seen by ANY pair, and the test says why: with the two tag bits
  of the lean strip's record left unswapped, Left and Top trade places in row1tag -- but a flipped column whose recorded cell
  took Left or Top always moves under the other penalty (left - p and top - p both change by del - ext, many EPSILONs), so the
  verdict never rests on that compare.  The test asserts that premise on every flipped column of the catalogue instead."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import advice_generic_model as gm  # noqa: E402

BY_NAME = {e[0]: e for e in gm.CATALOGUE}


def oracle_of(orc, entry):
    q, t, S, de, ex, pwm = gm.entry_pair(entry)
    if pwm:
        ref = orc.align_pwm(t, de, ex, S, want_matrices=True)
    else:
        ref = orc.align(orc.CORE_LOCAL, q, t, de, ex, S, want_matrices=True)
    assert ref["status"] == 0
    return ref


def assert_is_oracle(p, ref, M, where):
    assert np.array_equal(p["H"], ref["H"]), where
    assert np.array_equal(gm.TAG_TO_D[p["T"]][1:, 1:], ref["D"][1:, 1:]), where      # every tag, row 1 among them
    N = ref["H"].shape[1] - 1
    assert np.array_equal(p["z"][2:N + 1], ref["H"][M, 1:N] == 0), where


@pytest.mark.parametrize("entry", gm.CATALOGUE, ids=gm.IDS)
def test_catalogue_line_is_what_it_declares_and_converges_to_the_oracle(orc, entry):
    name, _, _, M, N, _, scheme, gaps, outcome, passes, props = entry
    q, t, S, de, ex, pwm = gm.entry_pair(entry)
    ref = oracle_of(orc, entry)
    p = gm.prediction(entry)
    assert (p["outcome"], p["passes"]) == (outcome, passes), (name, p["outcome"], p["passes"], p["moves"])
    assert p["word"] == (passes | (0x80 if outcome == "fallback" else 0))
    if outcome == "fallback":
        far = gm.predict_generic(q, t, S, de, ex, max_passes=64, pwm=pwm)
        assert far["outcome"] in ("consistent", "same") and far["passes"] > 4
        assert_is_oracle(far, ref, M, name)
    else:
        assert_is_oracle(p, ref, M, name)
    if outcome == "same":                                    # the soundness check, once more in the open
        H2, T2 = gm.spec_fill(q, t, S, de, ex, p["z"], pwm)
        assert np.array_equal(H2, p["H"]) and np.array_equal(T2, p["T"]) and np.array_equal(gm.observe(H2, M), p["z"])
        assert p["flips"][-1] and not p["movers"][-1]
    if outcome == "consistent":
        assert not p["flips"][-1]
    if "first" in props:
        assert p["passes"] >= 2 and p["moves"][0] == props["first"], (name, p["moves"])
    if "sole" in props:
        assert p["movers"][0] == [props["sole"]] and props["sole"] in p["flips"][0], (name, p["movers"][0])
    if "flips" in props:
        assert len(p["flips"][0]) > 0
    if "near" in props:
        assert gm.near_tie_cells_row1(ref["H"], q, t, S, de, ex, p["z"], pwm) > 0, name
    # max_passes 1..3: the strict-order routine exactly when the model needs more passes than it may make
    for k in (1, 2, 3):
        pk = gm.prediction(entry, k)
        if outcome != "fallback" and passes <= k:
            assert pk["word"] == passes, (name, k)
        else:
            assert pk["word"] == (k | 0x80), (name, k)
    assert gm.prediction(entry, 4)["word"] == p["word"]


def test_catalogue_covers_every_outcome_edge_and_route():
    got = {(e[8], e[9]) for e in gm.CATALOGUE}
    assert got >= {("consistent", 1), ("same", 1), ("consistent", 2), ("consistent", 3), ("consistent", 4), ("same", 2), ("same", 3),
                   ("same", 4), ("fallback", 4), ("no_hazard", 1)}
    firsts = {e[10].get("first") for e in gm.CATALOGUE}
    assert {"tag", "value"} <= firsts
    soles = {e[10]["sole"] for e in gm.CATALOGUE if "sole" in e[10]}
    assert {2, 63, 64, 65, 66, 127, 128, 129, 130} <= soles
    assert any(e[10].get("sole") == e[4] for e in gm.CATALOGUE)                              # x = N
    assert any(e[4] == 2 and e[9] >= 2 for e in gm.CATALOGUE) and any(e[4] == 1 for e in gm.CATALOGUE)
    assert any(e[7][0] == e[7][1] for e in gm.CATALOGUE)
    # recording edges: M = 1, M = 2, every R of a one-strip pair at 64 R - 63, 64 R - 1 and 64 R, two strips
    rows = {e[3] for e in gm.CATALOGUE if e[9] >= 2 or e[10].get("flips")}
    want = {1, 2, 513, 600} | {m for R in range(1, 9) for m in (64 * R - 63, 64 * R - 1, 64 * R)}
    assert want <= rows, sorted(want - rows)
    assert {gm.lean_r(m) for m in rows if m <= 512} == set(range(1, 9))
    # the one-workgroup route: R = 1 with two waves, R = 2, R = 4; a ring that wraps and one that does not; two passes each
    wg = {(e[3], e[4]): gm.wg_route(e[3], e[4]) for e in gm.CATALOGUE if e[9] >= 2 and e[8] != "fallback" and gm.wg_route(e[3], e[4])}
    assert {(65, 300), (600, 40), (600, 300), (1100, 40), (1100, 300)} <= set(wg)
    assert wg[(65, 300)] == (1, 128) and wg[(600, 300)] == (2, 320) and wg[(1100, 40)] == (4, 320)
    # the deciding columns sit in a pair the workgroup route takes with 128 threads: 129 is its last thread's column
    assert all(gm.wg_route(BY_NAME[n][3], BY_NAME[n][4]) == (1, 128) for n in ("k63", "k64", "k65", "k66", "k127", "k128", "k129", "k130"))
    fam = {e[6] for e in gm.CATALOGUE}
    assert fam >= {"pm1", "blosum", "blosum_half", "blosum_037", "tenths", "pwm_int", "pwm_real"}
    assert any(e[6] == "pm1" and e[7] == (1.5, 0.5) for e in gm.CATALOGUE)
    assert max(e[3] for e in gm.CATALOGUE) <= 1100 and max(e[4] for e in gm.CATALOGUE) <= 300


# defect: (the line that shows it, threads of the walk / rows per lane the defect needs, what goes wrong)
PLANTED = {
    "no_tag": ("c2", 64, "the tag compare dropped: a pass whose flip moves a direction alone is accepted"),
    "end_n_minus_1": ("xN", 64, "the loop ends at N - 1: the deciding flip at x = N is never seen"),
    "start_3": ("x2", 64, "the loop starts at 3: the deciding flip at x = 2 is never seen"),
    "stride_mix": ("k129", 128, "the one-wave walk under the workgroup's stride: columns 66 .. 129 of 128 threads are skipped"),
    "old_penalty": ("v2", 64, "the recheck under the OLD penalty reproduces the recorded cell: every pass is accepted"),
    "row1_x": ("rx", 64, "the recheck reads row1[x] for the left neighbour: a cell that moves through H[1][x-1] is accepted"),
    "lean_row_r": ("l100", 2, "the recorded tag is the lane's last row's: harmless flips look harmful, a pass too many"),
    "b_partial": ("bp", 64, "only the deciding bits are adopted: the next pass runs under an advice nobody observed"),
}


@pytest.mark.parametrize("defect", sorted(PLANTED))
def test_planted_defect_is_seen_by_a_named_line(orc, defect):
    name, nthreads, why = PLANTED[defect]
    entry = BY_NAME[name]
    q, t, S, de, ex, pwm = gm.entry_pair(entry)
    true = gm.prediction(entry)
    bad = gm.predict_generic(q, t, S, de, ex, pwm=pwm, defect=defect, nthreads=nthreads)
    ref = oracle_of(orc, entry)
    wrong_word = bad["word"] != true["word"]
    wrong_matrix = bad["outcome"] != "fallback" and not (np.array_equal(bad["H"], ref["H"]) and
                                                         np.array_equal(gm.TAG_TO_D[bad["T"]][1:, 1:], ref["D"][1:, 1:]))
    print(defect, name, "word", true["word"], "->", bad["word"], "matrix wrong" if wrong_matrix else "matrix right", "--", why)
    assert wrong_word, (defect, name)                        # the GPU test holds the word exactly: this is what it would see
    assert bad["outcome"] == "fallback" or wrong_matrix or bad["passes"] > true["passes"], (defect, name)
    if defect == "stride_mix":                               # the neighbours of the skipped range are still looked at
        for ok in ("k65", "k130"):
            e = BY_NAME[ok]
            q2, t2, S2, d2, e2, _ = gm.entry_pair(e)
            assert gm.predict_generic(q2, t2, S2, d2, e2, defect=defect, nthreads=128)["word"] == gm.prediction(e)["word"]
        for skipped in ("k66", "k127", "k128"):
            e = BY_NAME[skipped]
            q2, t2, S2, d2, e2, _ = gm.entry_pair(e)
            assert gm.predict_generic(q2, t2, S2, d2, e2, defect=defect, nthreads=128)["word"] == 1


def test_unswapped_lean_tag_bits_cannot_change_a_verdict():
    """`lean_unswapped` (row1tag = t where the lean strip writes ((t & 1) << 1) | (t >> 1)) trades Left and Top in the record.  No
    pair can show it through `passes`: at a flipped column whose recorded cell took Left or Top, the cell always moves under the
    other penalty, with either record.  Asserted on every flipped column of every pass of the catalogue, and the defect's
    prediction is the true one on every line."""
    seen = 0
    for e in gm.CATALOGUE:
        if e[3] > 130:
            continue
        q, t, S, de, ex, pwm = gm.entry_pair(e)
        true = gm.prediction(e)
        bad = gm.predict_generic(q, t, S, de, ex, pwm=pwm, defect="lean_unswapped")
        assert bad["word"] == true["word"] and bad["movers"] == true["movers"], e[0]
        b = np.zeros(len(true["z"]), dtype=bool)
        for k, flips in enumerate(true["flips"]):             # replay the passes: recorded tag of every flipped column
            H, T = gm.spec_fill(q, t, S, de, ex, b, pwm)
            z = gm.observe(H, e[3])
            for x in flips:
                if T[1, x] in (gm.TAG_LEFT, gm.TAG_TOP):
                    seen += 1
                    assert x in true["movers"][k], (e[0], k, x)
                b[x] = z[x]
    assert seen > 0
