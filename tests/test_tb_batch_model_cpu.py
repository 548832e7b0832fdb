"""tests/tb_batch_model.py and tests/tb_batch_cases.py held to the CPU oracle; no GPU.

* The restatement is right: the oracle's D, packed, walked by lane_walk and by wave_walk and expanded, gives the oracle's start cell,
  length and both strings, for every case and every layout and scheme the GPU test runs it with.
* The construction holds: every case meets its aim on the oracle's path, every group its group aims; nothing is left out.
* The cases discriminate: every variant of the model gives a wrong answer on at least one case aimed at the rule it breaks.
* Pins of the geometry: pack then dir_at returns D; the (65535 + R) / R multiply-shift is iy // R.
Printed: per aim the cases that meet it, per variant the cases that catch it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tb_batch_cases as tc  # noqa: E402
import tb_batch_model as bm  # noqa: E402
from aligner_amd import build as native_build  # noqa: E402

_refs = {}


def ref_of(orc, case, kind="int"):
    key = (case.id, kind)
    if key not in _refs:
        ref = tc.oracle(orc, case, kind, want_matrices=True)
        assert ref["status"] == 0, key
        ref.pop("H")
        _refs[key] = ref
    return _refs[key]


def answer(store, case, ref, variant=None, wave=True):
    """The model's (start, length, query string, target string, reads outside a sequence, records, rounds) of a case."""
    q, t = case.seqs()
    walk_v = variant if variant in bm.WALK_VARIANTS else None
    if wave:
        tags, start, n, recs, rounds = bm.wave_walk(store, ref["end"], case.mode(), case.legacy(), walk_v)
    else:
        tags, start, n, recs = bm.lane_walk(store, ref["end"], case.mode(), case.legacy(), walk_v)
        rounds = []
    qa, ta, outside = bm.expand(tags, start, q, t, variant=variant if variant in bm.EXPAND_VARIANTS else None)
    seed = ref["end"]
    return start, n, qa + [int(q[seed[1] - 1])], ta + [int(t[seed[0] - 1])], outside, recs, rounds


def want(ref):
    return ref["start"], len(ref["qa"]) - 1, ref["qa"].tolist(), ref["ta"].tolist()


def stores(case, ref):
    M, N = case.shape()
    if case.group == "ubatch":
        return [("ubatch", bm.pack(ref["D"], M, N, bm.UBATCH, tc.ubatch_r(M)))]
    out = [("skew", bm.pack(ref["D"], M, N))]
    if case.subset:
        out.append(("rowmajor", bm.pack(ref["D"], M, N, bm.ROWMAJOR)))
    return out


ALL = tc.cases() + tc.ubatch_cases()


def test_restatement_and_construction(orc):
    met, missed = {}, []
    group_seen = {}
    n_checked = 0
    for case in ALL:
        for kind in tc.kinds_of(case):
            ref = ref_of(orc, case, kind)
            for lname, store in stores(case, ref):
                for wave in (True, False):
                    got = answer(store, case, ref, wave=wave)
                    assert got[:4] == want(ref), (case.id, kind, lname, "wave" if wave else "lane", got[0], got[1], want(ref)[:2])
                    assert got[4] == 0, (case.id, "a read outside a sequence")
                    n_checked += 1
            first, moves = tc.moves_of(case, ref)
            _, _, _, _, _, recs, rounds = answer(stores(case, ref)[0][1], case, ref)
            miss = tc.check_aim(case, ref, moves, recs, rounds)
            if miss:
                missed.append((case.id, kind, miss))
            if kind == tc.kinds_of(case)[0]:
                for name in case.aim:
                    met.setdefault(name, []).append(case.id)
                g = group_seen.setdefault(case.group, dict(served=set(), reasons=set(), clamp=False))
                g["served"] |= {r["reg"] for r in recs}
                g["reasons"] |= {r["reason"] for r in rounds}
                g["clamp"] |= any(r["clamp"] for r in rounds)
    for name in tc.AIM_NAMES:
        print("aim %-16s %3d cases: %s" % (name, len(met.get(name, [])), " ".join(met.get(name, [])[:6])))
    print("%d walks checked over %d cases" % (n_checked, len(ALL)))
    for m in missed:
        print("MISSED", m)
    assert not missed, missed[:5]
    for name in tc.AIM_NAMES:
        assert met.get(name), "no case aims at %s" % name
    for group, aims in tc.GROUP_AIMS.items():
        g = group_seen[group]
        print("group %s: served %s, reasons %s, clamp %s" % (group, sorted(g["served"]), sorted(g["reasons"]), g["clamp"]))
        assert aims["served"] <= g["served"] and aims["reasons"] <= g["reasons"] and g["clamp"] == aims["clamp"], (group, g)


def test_two_pairs_per_wave_batches_hold_every_case_in_both_halves():
    """No GPU: the batches of the GPU test between them hold every case of ubatch_cases(), each once in either half of a wave."""
    seen = {}
    for mode in tc.UBATCH_MODES:
        pairs, at, _, (S, _, _) = tc.batch_of(mode)
        half = tc.duo_halves(pairs)
        assert len(pairs) >= 3100 and max(int(max(q.max(), t.max())) for q, t in pairs) < S.shape[0]
        for pos, c in at.items():
            assert (pairs[pos][0] == c.seqs()[0]).all() and (pairs[pos][1] == c.seqs()[1]).all()
            seen.setdefault(c.id, set()).add(half[pos])
    assert seen == {c.id: {0, 1} for c in tc.ubatch_cases()}, seen


def test_subset_holds_a_case_of_every_aim():
    aims = {name for c in tc.cases() for name in c.aim}
    sub = {name for c in tc.cases() if c.subset for name in c.aim}
    assert aims - {"end_row"} <= sub, aims - sub          # (end_row: legacy local only, the batch fast kernel)


# the groups whose cases are aimed at the rule a variant breaks
VARIANT_GROUPS = {"window2": ("window",), "no_wrap_recentre": ("window",), "flush63": ("tags", "border"), "no_lend": ("lastblock", "strips"),
                  "stale_strip": ("strips",), "last_r8": ("strips", "window", "lastblock"), "no_carry": ("tags",), "tag3_moves": ("tags", "lastblock")}


def test_cases_discriminate(orc):
    assert set(VARIANT_GROUPS) == set(bm.VARIANTS)
    for variant in bm.VARIANTS:
        caught = []
        for case in tc.cases():
            if case.group not in VARIANT_GROUPS[variant]:
                continue
            ref = ref_of(orc, case)
            store = stores(case, ref)[0][1]
            for wave in (True,) if variant in bm.WAVE_ONLY else (True, False):
                try:
                    got = answer(store, case, ref, variant, wave)
                except IndexError:                       # a lane or a word that does not exist: the kernel's read out of bounds
                    got = None
                how = "index" if got is None else "answer" if got[:4] != want(ref) else "read" if got[4] else None
                if how:
                    caught.append((case.id, how))
                    break
        for how, what in (("answer", "a wrong start cell, length or string"), ("read", "a read outside a sequence, the strings right"),
                          ("index", "a lane or word that does not exist")):
            ids = [c for c, h in caught if h == how]
            print("variant %-18s %-45s %3d cases: %s" % (variant, what, len(ids), " ".join(ids[:8])))
        # What the GPU test can see is a wrong answer.  tag3_moves leaves every string right (a padded group is the last one) and shows
        # as a load past a sequence; stale_strip takes the lane number past 63 wherever a strip with another R is entered, so the
        # kernel would read another lane's or another pair's words and there is no defined answer to compare.
        kind = {"tag3_moves": "read", "stale_strip": "index"}.get(variant, "answer")
        assert [c for c, h in caught if h == kind], "no case catches the variant %s" % variant


def test_pwm_windows_restated(orc):
    for real in (True, False):
        pwm, dele, ext, wins = tc.pwm_cases(real)
        lengths = set()
        for name, seq in wins:
            ref = orc.align_pwm(seq, dele, ext, pwm, want_matrices=True)
            assert ref["status"] == 0
            store = bm.pack(ref["D"], len(seq), tc.PWM_COLS)
            first, moves = bm.path_from_alignment(False, ref["end"], ref["start"], ref["numbered"], ref["qal"], pwm=True)
            lengths.add(len(moves))
            for walk in (bm.wave_walk, bm.lane_walk):
                tags, start, n = walk(store, ref["end"], bm.LOCAL)[:3]
                assert (start, n, tags) == (ref["start"], len(moves), [bm.TAG[m] for m in moves]), (name, real)
                numbered, qal, outside = bm.expand(tags, start, None, seq, pwm=True)
                assert numbered == ref["numbered"].tolist() and qal == ref["qal"].tolist() and outside == 0, (name, real)
        print("pwm %s: path lengths %s" % ("real" if real else "int", sorted(lengths)))
        assert min(lengths) <= 64 and any(64 < n <= 128 for n in lengths) and max(lengths) > 128, lengths


@pytest.mark.parametrize("M", [1, 63, 64, 65, 511, 512, 513])
def test_pack_then_dir_at_returns_D(M):
    rng = np.random.default_rng(M)
    for N in (1, 2, 15, 16, 17, 70):
        D = rng.integers(0, 4, (M + 1, N + 1)).astype(np.uint8)
        layouts = [(bm.SKEW, 0), (bm.ROWMAJOR, 0)] + [(bm.UNIFORM, R) for R in range(1, 9)]
        cells = [(y, x) for y in range(1, M + 1) for x in range(1, N + 1)]
        if len(cells) > 3000:
            edge = [c for c in cells if c[0] in (1, 2, 8, 9, 64, 65, 448, 449, 504, 505, 511, 512, 513) or c[0] >= M - 1]
            pick = rng.choice(len(cells), 1200, replace=False)
            cells = edge + [cells[i] for i in pick]
        for layout, R in layouts:
            store = bm.pack(D, M, N, layout, R)
            for y, x in cells:
                assert store.dir_at(y, x, True) == D[y, x], (M, N, layout, R, y, x)
            assert store.dir_at(0, 1, True) == 1 and store.dir_at(1, 0, True) == 0 and store.dir_at(0, 0, True) == 3 and store.dir_at(0, 1, False) == 3


def test_multiply_shift_is_the_division():
    for R in range(1, 9):
        rinv = (65535 + R) // R
        assert all((iy * rinv) >> 16 == iy // R for iy in range(512)), R
    assert [bm.spb(R) for R in range(1, 9)] == [16, 8, 4, 4, 2, 2, 2, 2]
    assert "aln_traceback.hip" in native_build.SOURCES and "aln_launch.h" in native_build.HEADERS     # where the walks restated here live
