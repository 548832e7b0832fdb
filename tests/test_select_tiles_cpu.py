"""The constructions of tests/select_cases.py against the CPU oracle: the scores they assume, and that the planted positions cover
the thread, tile and 256-tile edges the GPU tests (test_select_tiles_gpu.py) are about.  This is what makes the kept sets of those
tests known in advance."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import select_cases as SC                                                        # noqa: E402
import seqset_ref                                                                # noqa: E402


def test_scan_scores_rise_with_the_run(orc):
    m = SC.scan_pwm()
    f = []
    for L in range(SC.W + 1):
        r = orc.align_pwm(SC.window_content(L), SC.DEL, SC.EXT, m)
        assert r["status"] == 0
        assert r["f"] == SC.F_OF_RUN[L], L
        f.append(r["f"])
    assert all(a < b for a, b in zip(f, f[1:]))              # strictly increasing in L; the unplanted window (L = 0) is the lowest
    # a run changes its own window only: windows do not overlap, and a window's f depends on its 8 residues
    case, _ = SC.case_edges()
    assert case.step == case.width == SC.W and len(case.strand) == case.n * SC.W
    assert {k: int(L) for k, L in enumerate(case.runs) if L} == case.planted


def test_scan_thresholds_are_exact_and_differ():
    case, named = SC.case_edges()
    f = case.f()
    sets = []
    for (mean, sd, z), min_run in SC.SCAN_THRESHOLDS:
        got = SC.numpy_kept(f, mean, sd, z)
        want = case.kept(min_run) if min_run is not None else np.zeros(0, dtype=np.int64)
        assert got.tolist() == want.tolist(), (mean, sd, z)
        sets.append(got.tolist())
    assert len({tuple(s) for s in sets[:3]}) == 3 and all(len(s) for s in sets[:4]) and not sets[4] and not sets[5]
    # the thresholds that hold exactly: z == z_min at that run, in floating point
    assert (SC.F_OF_RUN[1] - 0.0) / 1.0 == 1.0 and (SC.F_OF_RUN[4] - 1.0) / 2.0 == 1.5 and (SC.F_OF_RUN[7] - 0.5) / 0.25 == 26.0
    assert (case.runs == 4).any() and (case.runs == 7).any() and (case.runs == 3).any()       # 0 / 0 occurs under sd = 0


def test_scan_cases_cover_the_edges():
    T = SC.TILE
    case, named = SC.case_edges()
    assert case.n == 3 * T + 5 and case.tiles == 4
    assert named == [0, 7, 8, T - 1, T, T + 1, 2 * T - 1, 2 * T, 3 * T - 1, 3 * T, case.n - 1]
    assert all(k in case.planted for k in named)
    counts = case.tile_counts(1)
    print("edges: tile counts", counts.tolist(), "planted", len(case.planted))
    assert len(set(counts.tolist())) >= 3 and counts.min() >= 1                   # tile counts differ
    assert 60 <= len(case.planted) <= 80                                          # about 1 %
    assert set(case.planted.values()) == set(range(1, SC.W + 1))
    cuts = SC.capacity_cuts(case)
    assert cuts == [counts[0], counts[0] + 1, counts[0] - 1, counts.sum() - 1, counts.sum()] and min(cuts) >= 8
    kept = case.kept(1)
    assert kept[cuts[0] - 1] == T - 1 and kept[cuts[0]] == T                      # the first cut falls exactly between two tiles

    case = SC.case_empty_tiles()
    counts = case.tile_counts(1)
    assert case.tiles == 4 and counts.tolist() == [0, 0, len(case.planted), 0] and counts[2] >= 20
    assert 2 * T in case.planted and 3 * T - 1 in case.planted

    case = SC.case_exact_multiple()
    assert case.n % T == 0 and case.n - 1 in case.planted and case.tile_counts(1)[0] == 0

    case, named = SC.case_many_tiles()
    n = case.n
    assert n == 257 * T + 5 == 526341 and len(case.strand) == SC.MANY_TILES_LEN == 4210728 and case.tiles == 258
    assert named == [0, 256 * T - 1, 256 * T, 256 * T + 1, n - 1] == [0, 524287, 524288, 524289, 526340]
    assert all(case.planted[k] >= 2 for k in named)
    strong = case.tile_counts(2)
    print("many tiles: runs >= 2:", int(strong.sum()), "per tile", int(strong.min()), "..", int(strong.max()))
    assert 2500 <= strong.sum() <= 3500 and strong.min() == 0 and 30 <= strong.max() <= 45
    assert strong[256] >= 2 and strong[257] >= 1 and strong[255] >= 1
    listed = len(case.kept(1))
    print("many tiles: runs >= 1:", listed)
    assert listed > 16384 and listed % 16 != 0                                    # beyond the frequency kernel's grid cap, a short last run
    grid = min((listed + 15) // 16, 1024)
    per = (listed + grid - 1) // grid
    assert per > 16 and (listed + per - 1) // per < 1024 and listed % per != 0
    for name, keep in SC.keep_lists(listed).items():
        assert len(keep) > 16384, name
    doubled = SC.keep_lists(listed)["doubled"]
    assert np.bincount(doubled, minlength=listed).tolist() == [2 if i % 3 == 0 else 1 for i in range(listed)]


def test_set_scores_by_content(orc, blosum62):
    from aligner_amd.enums import Protein
    codes = [np.asarray(Protein.str_to_vec(s), dtype=np.uint8) for s in SC.CONTENTS]
    for a, q in enumerate(codes):
        for b, t in enumerate(codes):
            o = orc.align(orc.CORE_LOCAL, q, t, SC.SET_DEL, SC.SET_EXT, blosum62)
            assert o["status"] == SC.PAIR_STATUS[a, b], (a, b)
            assert o["f"] == SC.PAIR_F[a, b], (a, b)
    ok = SC.PAIR_STATUS == SC.OK
    marked = SC.CONTENTS.index("WWWW")
    others = ok.copy()
    others[marked, marked] = False
    assert ok[marked, marked] and SC.PAIR_F[marked, marked] == SC.F_MARKED > SC.PAIR_F[others].max()
    assert (SC.PAIR_F[others] == SC.F_BACKGROUND).sum() == 1                      # one background score equals the second threshold
    assert (SC.PAIR_STATUS[SC.CONTENTS.index("")] == SC.ERR_EMPTY).all() and (SC.PAIR_STATUS[:, SC.CONTENTS.index("")] == SC.ERR_EMPTY).all()


def test_set_marked_pairs_cover_the_tiles():
    T, S = SC.TILE, SC.S
    assert S * S == 527076 and (S * S + T - 1) // T == 258
    q, t, f, status = SC.block_expect(("full",))
    assert np.array_equal(q * S + t, np.arange(S * S))
    hits = SC.expect_hits(f, status, SC.F_MARKED)
    assert len(hits) == len(SC.MARKED) ** 2
    assert {(int(a), int(b)) for a, b in zip(q[hits], t[hits])} == {(a, b) for a in SC.MARKED for b in SC.MARKED}
    tiles = sorted(set((hits // T).tolist()))
    print("set: marked pairs", len(hits), "in tiles", tiles)
    assert 2 * S + 595 == 2047 and 2 * S + 596 == 2048 and {2047, 2048} <= set(hits.tolist())            # tile 0 | tile 1
    assert 722 * S + 115 == 256 * T - 1 and 722 * S + 116 == 256 * T and {256 * T - 1, 256 * T} <= set(hits.tolist())
    assert {0, 1, 255, 256, 257} <= set(tiles)
    # the empty sequence: its row and its column lie in tiles 256 and 257, and every pair with it fails
    bad = np.flatnonzero(status == SC.ERR_EMPTY)
    assert len(bad) == 2 * S - 1
    row = bad[q[bad] == SC.EMPTY]
    assert len(row) == S and (row // T >= 256).all()
    assert {int(k) // T for k in bad[(t[bad] == SC.EMPTY) & (q[bad] >= 722)]} == {256, 257}
    assert (status == SC.ERR_NO_POSITIVE).sum() == 2 * len(SC.MARKED) * (S - 1 - len(SC.MARKED))
    # the background threshold keeps whole runs of pairs in every tile, with differing counts
    back = SC.expect_hits(f, status, SC.F_BACKGROUND)
    per_tile = np.bincount(back // T, minlength=258)
    print("set: f >= 12 keeps", len(back), "per tile", int(per_tile.min()), "..", int(per_tile.max()))
    assert per_tile.min() > 0 and len(set(per_tile.tolist())) > 5
    # the tail rectangle: about 3 tiles, with the empty row, failed pairs and hits on its tile edges' both sides somewhere
    qr, tr, fr, sr = SC.block_expect(("rect",) + SC.RECT_TAIL)
    assert len(qr) == 5808 and 2 * T < len(qr) < 3 * T and (qr == SC.EMPTY).sum() == S
    everything = SC.expect_hits(fr, sr, float("-inf"))
    assert 0 < len(everything) < len(qr) and (sr[everything] == SC.OK).all() and (sr != SC.OK).sum() == len(qr) - len(everything)
    assert (sr[2 * T:] != SC.OK).any() and (sr[:T] != SC.OK).any()
    # the inner rectangle and the triangle hold marked pairs, in the order of tests/seqset_ref.py
    qi, ti, fi, si = SC.block_expect(("rect",) + SC.RECT_INNER)
    assert qi[0] == 590 and ti[0] == 110 and len(qi) == 136 * 490
    inner = SC.expect_hits(fi, si, SC.F_MARKED)
    assert {(int(a), int(b)) for a, b in zip(qi[inner], ti[inner])} == {(a, b) for a in (595, 596, 722, 725) for b in (115, 116, 595, 596)}
    assert len({int(k) // T for k in inner}) >= 3
    qu, tu, fu, su = SC.block_expect(("upper", 0, S))
    up = SC.expect_hits(fu, su, SC.F_MARKED)
    assert len(qu) == S * (S - 1) // 2 and len(up) == len(SC.MARKED) * (len(SC.MARKED) - 1) // 2
    assert [seqset_ref.upper_rank(0, S, int(a), int(b)) for a, b in zip(qu[up], tu[up])] == up.tolist()
    assert len({int(k) // T for k in up}) >= 4


def test_chunked_run_cuts_off_the_tile_edges():
    L = SC.set_lengths()
    target = SC.chunk_cells()
    for block in (("full",), ("upper", 0, SC.S)):
        q, t, f, status = SC.block_expect(block)
        counts = SC.chunk_counts(L, q, t, float(target))
        print("chunks of", block[0], counts)
        assert sum(counts) == len(q) and len(counts) >= 3
        assert all(c % SC.TILE != 0 and c > 4 * SC.TILE for c in counts)          # several tiles each, ending off a tile boundary
        k0 = np.cumsum(counts)[:-1]
        assert all(int(k) % SC.TILE != 0 for k in k0)
    # a literal restatement of the chunking loop agrees with the vectorised one on a small block
    q, t, f, status = SC.block_expect(("rect",) + SC.RECT_TAIL)
    cells = (L[q] * L[t]).astype(float)
    for target in (900.0, 2500.0, 1e9):
        total, out, acc, done, n = cells.sum(), [], 0.0, 0.0, 0
        if total <= 1.5 * target:
            out = [len(cells)]
        else:
            for k in range(len(cells)):
                acc += cells[k]
                n += 1
                if acc >= target and (total - done - acc >= 0.25 * target or k + 1 == len(cells)):
                    out.append(n)
                    done += acc
                    acc, n = 0.0, 0
            if n:
                out.append(n)
        assert SC.chunk_counts(L, q, t, target) == out, target
