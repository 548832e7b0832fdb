"""The restated rule of the single-pair traceback (tests/tb_single_model.py) on hand-made paths, and every constructed case of
tests/tb_single_cases.py on the oracle's own path: a case that misses the class, the offset or the window flag it is built for
fails here, on the CPU, so that no GPU test can pass for a reason other than the one its name gives."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tb_single_cases as tc  # noqa: E402
import tb_single_model as model  # noqa: E402

CASES = tc.cases()


def rec(strip, cls, entry, delta, steps, interior, seg=False, mapw=False, gave_up=False):
    if cls in (1, 3):
        mapw = gave_up = None
    return dict(strip=strip, cls=cls, entry=entry, delta=delta, steps=steps, interior=interior, seg_leaves_window=seg,
                map_leaves_window=mapw, map_gave_up=gave_up)


def test_pure_diagonal():
    """200 x 200, R = 1: eight rows of strip 3, then three whole strips on the line."""
    got = model.classify(model.LOCAL, 200, 200, 1, (200, 200), ["D"] * 200)
    assert got == [rec(3, 1, (200, 200), None, 8, 8), rec(2, 2, (192, 192), 0, 64, 64), rec(1, 2, (128, 128), 0, 64, 64),
                   rec(0, 2, (64, 64), 0, 64, 64)]
    assert model.class_string(got, 200, 1) == "2221"
    # R = 2: strips of 128 rows
    got = model.classify(model.LOCAL, 200, 200, 2, (200, 200), ["D"] * 200)
    assert got == [rec(1, 1, (200, 200), None, 72, 72), rec(0, 2, (128, 128), 0, 128, 128)]


def test_one_left_run():
    """128 x 1000: 800 columns to the left on row 96.  The walk's own strip drops from wave step 1062 (quad 16: the window starts at
    quad 5, step 320) to step 198; the strip above is entered 800 columns left of the line, outside the band [424, 1000]."""
    moves = ["D"] * 32 + ["L"] * 800 + ["D"] * 96
    got = model.classify(model.LOCAL, 128, 1000, 1, (128, 1000), moves)
    assert got == [rec(1, 1, (128, 1000), None, 864, 864, seg=True), rec(0, 3, (64, 136), -800, 64, 64)]
    assert model.class_string(got, 128, 1) == "31"
    assert model.band(128, 1000, 64, 1000) == (424, 1000)
    # 300 columns: inside the band, but 64 + 300 steps > the cap of 192 ... at R = 1 only when the run is in an entered strip
    moves = ["D"] * 96 + ["L"] * 300 + ["D"] * 32
    got = model.classify(model.LOCAL, 128, 1000, 1, (128, 1000), moves)
    assert got == [rec(1, 1, (128, 1000), None, 64, 64), rec(0, 4, (64, 936), 0, 364, 364, gave_up=True)]
    # exactly at the cap: 64 + 128 = 192 steps leave the strip with the last one allowed
    for run, cls in ((127, 2), (128, 2), (129, 4)):
        moves = ["D"] * 96 + ["L"] * run + ["D"] * 32
        got = model.classify(model.LOCAL, 128, 1000, 1, (128, 1000), moves)
        assert got[1] == rec(0, cls, (64, 936), 0, 64 + run, 64 + run, gave_up=cls == 4), run


def test_one_top_run_across_three_strips():
    """300 x 100: 200 rows up at column 80.  The line reaches column 0 at row 200, so every band is [0, 100]."""
    moves = ["D"] * 20 + ["T"] * 200 + ["D"] * 80
    got = model.classify(model.LOCAL, 300, 100, 1, (300, 100), moves)
    assert got == [rec(4, 1, (300, 100), None, 44, 44), rec(3, 2, (256, 80), 24, 64, 64), rec(2, 2, (192, 80), 88, 64, 64),
                   rec(1, 2, (128, 80), 152, 64, 64), rec(0, 2, (64, 64), 200, 64, 64)]
    assert model.class_string(got, 300, 1) == "22221"


def test_border_runs():
    """Global 150 x 100: column 0 is reached on row 120, Top from there: 56 border steps in strip 1, the whole of strip 0.
    Global 100 x 300: row 0 is reached at column 200, the Left run belongs to strip 0."""
    moves = ["D"] * 30 + ["L"] * 70 + ["T"] * 120
    got = model.classify(model.GLOBAL, 150, 100, 1, (150, 100), moves)
    assert got == [rec(2, 1, (150, 100), None, 22, 22), rec(1, 2, (128, 78), 0, 134, 78), rec(0, 2, (64, 0), -14, 64, 0)]
    moves = ["D"] * 100 + ["L"] * 200
    got = model.classify(model.GLOBAL, 100, 300, 1, (100, 300), moves)
    assert got == [rec(1, 1, (100, 300), None, 36, 36), rec(0, 2, (64, 264), 0, 264, 64)]
    # a walk that starts on a border of the local semantics visits nothing
    assert model.classify(model.LOCAL, 200, 1400, 1, (0, 1399), []) == []
    assert model.class_string([], 200, 1) == "0000"


def test_map_walk_leaves_the_window_from_a_block_s_low_columns():
    """R = 4, strip 0 of 512 x 2000 entered on the line at column 1256 -- the lowest column of its block of the band [744, 1767], whose
    window ends with the quad of step 1510 + 63 (quad 98: it starts at quad 51, step 816): 256 diagonal steps of 1.25 wave steps and
    300 to the left end near step 700, below it.  Entered one column left of the line the same column is its block's highest, the
    window ends with its own step 1318 (quad 82: from step 560) and the same walk stays inside."""
    moves = ["D"] * 300 + ["L"] * 300 + ["D"] * 212
    got = model.classify(model.LOCAL, 512, 2000, 4, (512, 1512), moves)
    assert [r["cls"] for r in got] == [1, 2] and got[1]["delta"] == 0 and got[1]["interior"] == 556 and got[1]["entry"] == (256, 1256)
    assert got[1]["map_leaves_window"] is True and got[1]["seg_leaves_window"] is False
    moves = ["D"] * 100 + ["L"] + ["D"] * 200 + ["L"] * 300 + ["D"] * 212
    got = model.classify(model.LOCAL, 512, 2000, 4, (512, 1513), moves)
    assert got[1]["entry"] == (256, 1256) and got[1]["delta"] == -1 and got[1]["cls"] == 2
    assert got[1]["map_leaves_window"] is False and got[1]["seg_leaves_window"] is False


def test_path_from_alignment():
    q = [5, 6, 98, 7, 7]        # forward strings, the last column is the duplicated seed pair
    t = [5, 98, 3, 7, 7]
    assert model.path_from_alignment(False, (3, 3), (0, 0), q, t) == ((3, 3), ["D", "T", "L", "D"])
    assert model.path_from_alignment(True, (4, 4), (0, 0), q, t) == ((3, 3), ["D", "T", "L", "D"])
    assert model.path_from_alignment(False, (2, 2), (0, 0), [1, 0, 2], [3, 3, 98], pwm=True) == ((2, 2), ["L", "T", "D"])


_cache = {}


def modelled(orc, case):
    if case.id not in _cache:
        ref = tc.oracle(orc, case)
        assert ref["status"] == 0
        _cache[case.id] = tc.run_model(case, ref)
    return _cache[case.id]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_hits_what_it_is_built_for(orc, case):
    strips, classes, moves = modelled(orc, case)
    q, t = case.seqs()
    assert len(q) <= 3000 and len(t) <= 3000
    if case.route == "single":      # the routing rule of a one-pair call
        assert len(q) >= 64 and len(t) >= 128 and len(q) * len(t) >= 1 << 18
    else:
        assert 65 <= len(t) <= 2048 and len(q) >= 16 and (len(t) + 64 * case.R - 1) // (64 * case.R) <= 16
    miss = tc.check_aim(case, strips, classes, moves)
    assert not miss, (case.id, miss, classes)


def test_pwm_case(orc):
    seq, pwm = tc.pwm_case()
    ref = orc.align_pwm(seq, tc.PWM_DEL, tc.PWM_EXT, pwm)
    strips, classes, moves = tc.pwm_model(ref)
    assert ref["status"] == 0 and len(seq) == 1500 and pwm.shape == (4, 400)
    # (the oracle's running gap penalty makes a gap after any aligned cell cost `ext` a cell, so it spreads the 200 missing columns
    # over the window's random residues instead of one run: the path is what the oracle says, with gaps of both kinds)
    assert "L" in moves and "T" in moves and len(moves) > 400
    assert "2" in classes and classes.count("1") == 1
