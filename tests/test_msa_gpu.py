"""Family alignments on the device (aln_seqset_held_msa_plan / _fill, HeldHits.msa) against the plain Python rule of msa_ref.py fed from
held.strings() and the summaries of the same held pass: every matrix, row list, record and counter for equality, no family and no hit
left out, and the properties of a family alignment asserted on the reference on the way.  Every test first asserts on the reference's
strings that the case it is named after is really there."""
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
import msa_ref as R  # noqa: E402
from aligner_amd import _ffi, allpairs, msa, profile, runtime  # noqa: E402
from aligner_amd import build as native_build  # noqa: E402
from aligner_amd.enums import Protein  # noqa: E402
from aligner_amd.fasta import encode_records, read_fasta  # noqa: E402
from aligner_amd.matrices import get_blosum62  # noqa: E402
from aligner_amd.seqset import SeqSet, rectangle  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLANK = 98
F_MIN = 200.0                 # the threshold at which cluster_cases.family_set falls into families and loners
FILTER = dict(min_identity=0.5, min_q_cover=0.5)
DEL, EXT = 4.0, 1.0           # low gap costs for the hand-built families: their inserts are bridged, not cut


def check(held, labels, centers=None, matrix=None, **th):
    """HeldHits.msa against the reference over held.strings(); returns (FamilyAlignments, the reference's (mats, lists, recs, summary),
    (summaries, strings, sequences))"""
    ss = held.owner
    got = held.msa(labels, centers=centers, matrix=matrix, **th)
    fill_stats = ss.stats()
    kept = held.filter(matrix, **th) if matrix is not None else None
    lab = profile.labels_of(labels)
    mats, lists, recs, summ, (res, strs, seqs) = R.from_held(held, lab, got.centers, BLANK, kept)
    assert (res["status"] == 0).all()
    want_out, want_rows = R.flat(mats, lists)
    assert got.summary == summ and got.summary["overflow"] == 0
    assert [tuple(int(x) for x in r) for r in got.records.tolist()] == recs
    assert got.out.dtype == np.uint8 and got.out.tobytes() == want_out.tobytes()
    assert got.row_hit.dtype == np.uint32 and got.row_hit.tolist() == want_rows.tolist()
    assert len(got) == len(mats) == len(got.centers)
    for i, (m, rows) in enumerate(zip(mats, lists)):                  # the views, family by family
        assert got.rows(i).shape == m.shape and got.rows(i).tolist() == m.tolist() and got.hits(i).tolist() == rows[1:]
        c = int(got.centers[i])
        assert got.members(i).tolist() == [c] + [int(held.t[h]) if int(held.q[h]) == c else int(held.q[h]) for h in rows[1:]]
    assert sum(len(l) - 1 for l in lists) == summ["contributing"]      # every contributing hit is a row of some family
    R.check_properties(mats, lists, recs, held.q, held.t, res, strs, seqs, BLANK)
    plan = held.last_msa_plan_stats
    bits = 4 * ((matrix.size + 31) // 32) if matrix is not None and len(held) else 0
    assert plan["bytes_up"] == 8 * len(held) + 4 * len(ss) + 12 * len(got.centers) + bits and plan["bytes_down"] == 16 * len(got.centers) + 64
    assert fill_stats["bytes_up"] == 16 * len(got.centers) and fill_stats["bytes_down"] == summ["bytes"] + 4 * summ["total_rows"]
    return got, (mats, lists, recs, summ), (res, strs, seqs)


def centre_runs(cs, n):
    """[(first column, length, residues in front)] of the maximal runs of blanks among the first n columns of a centre's string"""
    runs, j, seen = [], 0, 0
    while j < n:
        if cs[j] == BLANK:
            k = j
            while k < n and cs[k] == BLANK:
                k += 1
            runs.append((j, k - j, seen))
            j = k
        else:
            j += 1
            seen += 1
    return runs


def runs_of(held, res, strs, c=0):
    """per hit of centre c: its runs"""
    out = []
    for h in range(len(held)):
        if int(held.q[h]) == c or int(held.t[h]) == c:
            cs = strs[h][0] if int(held.q[h]) == c else strs[h][1]
            out.append(centre_runs(cs, R.counted_columns(int(res["aln_len"][h]))))
    return out


# ---------------------------------------------------------------- wave rounds: runs across and beyond a round of 64 columns
def test_runs_across_the_rounds():
    rng = np.random.default_rng(64)
    centre = rng.integers(0, 20, size=150).astype(np.uint8)
    recs = [centre]
    for at, width in ((61, 6), (60, 4), (62, 3), (63, 1), (64, 2), (75, 70), (40, 130), (126, 5)) + tuple((at, 3) for at in range(57, 68)):
        recs.append(np.insert(centre, at, rng.integers(0, 20, size=width).astype(np.uint8)))
    recs.append(np.delete(centre, np.arange(60, 68)))
    recs.append(np.insert(np.delete(centre, np.arange(20, 24)), 57, rng.integers(0, 20, size=9).astype(np.uint8)))
    S = get_blosum62()
    with SeqSet(recs) as ss:
        held = ss.hits(S, DEL, EXT, 200.0, rectangle(0, 1, 1, len(recs) - 1))
        res, strs = held.strings()
        assert len(held) == len(recs) - 1 and (res["aln_len"] > 128).all()
        runs = [r for hit_runs in runs_of(held, res, strs) for r in hit_runs]
        assert any(a <= 63 and a + n > 64 for a, n, _b in runs), "a run lies across columns 63 / 64"
        assert any(n > 64 for a, n, _b in runs), "a run is longer than a round"
        assert any(a == 64 for a, n, _b in runs) and any(a + n == 64 for a, n, _b in runs)
        got, (mats, lists, recs_w, summ), _ = check(held, np.zeros(len(recs), dtype=np.uint32))
        assert got.centers.tolist() == [0] and summ["contributing"] == len(held) and int(got.records["inserted"][0]) >= 70
        # the centre as the target of every hit: the same family, the other string
        held = ss.hits(S, DEL, EXT, 200.0, rectangle(1, len(recs) - 1, 0, 1))
        other, _w, _ = check(held, np.zeros(len(recs), dtype=np.uint32))
        assert int(other.records["width"][0]) == int(got.records["width"][0]) and other.rows(0)[0].tolist() == got.rows(0)[0].tolist()


# ---------------------------------------------------------------- global semantics: inserts before position 0 and after the last residue
def test_global_overhangs():
    rng = np.random.default_rng(5)
    centre = rng.integers(0, 20, size=70).astype(np.uint8)
    recs = [centre, np.concatenate([rng.integers(0, 20, size=5), centre, rng.integers(0, 20, size=4)]).astype(np.uint8),
            np.concatenate([rng.integers(0, 20, size=2), centre[:30], centre[33:], rng.integers(0, 20, size=7)]).astype(np.uint8), centre[3:60].copy()]
    S = get_blosum62()
    with SeqSet(recs) as ss:
        held = ss.hits(S, 4.0, 4.0, 0.0, rectangle(0, 4, 0, 4), semantics=_ffi.CORE_GLOBAL)      # (the global scheme of tests/test_seqset_gpu.py)
        assert len(held) == 16
        res, strs = held.strings()
        first = [r for r in runs_of(held, res, strs) if r and r[0][0] == 0]
        assert first, "a hit begins with an insert"
        got, (mats, lists, recs_w, summ), _ = check(held, np.zeros(4, dtype=np.uint32))
        m = mats[0]
        assert m[0, 0] == BLANK and m[0, -1] == BLANK, "an insert before position 0 and one after the last residue"
        assert (m[1:, 0] != BLANK).any() and (m[1:, -1] != BLANK).any() and (m[1:, 0] == BLANK).any()
        assert summ["self_pairs"] == 4 and summ["between_members"] == 6 and summ["contributing"] == 6      # both orientations: two rows a pair
        assert int(got.records["rows"][0]) == 6 and int(got.records["inserted"][0]) >= 2


# ---------------------------------------------------------------- a centre beyond one trip of the layout scan
def test_inserts_beyond_position_256():
    rng = np.random.default_rng(256)
    centre = rng.integers(0, 20, size=330).astype(np.uint8)
    recs = [centre]
    for at, width in ((100, 3), (255, 2), (256, 4), (256, 2), (256, 3), (257, 1), (300, 6), (329, 2)):
        recs.append(np.insert(centre, at, rng.integers(0, 20, size=width).astype(np.uint8)))
    recs.append(np.insert(np.insert(centre, 310, [1, 2, 3]), 40, [4, 5]).astype(np.uint8))
    S = get_blosum62()
    with SeqSet(recs) as ss:
        held = ss.hits(S, DEL, EXT, 300.0, rectangle(0, 1, 1, len(recs) - 1))
        assert len(held) == len(recs) - 1
        got, (mats, lists, recs_w, summ), _ = check(held, np.zeros(len(recs), dtype=np.uint32))
        row0 = mats[0][0]
        col = np.flatnonzero(row0 != BLANK)
        blanks = np.flatnonzero(row0 == BLANK)
        assert len(col) == 330 and (blanks > col[256]).sum() >= 6 and (blanks < col[255]).sum() >= 3, "inserts on both sides of position 256"
        assert ((blanks > col[255]) & (blanks < col[256])).any(), "an insert before position 256 itself"


# ---------------------------------------------------------------- contention on the max, ranks beyond 64 and 256 entries
def test_one_family_of_300_members():
    rng = np.random.default_rng(300)
    centre = rng.integers(0, 20, size=48).astype(np.uint8)
    recs = [centre]
    for k in range(300):
        m = centre.copy()
        hit = rng.random(48) < 0.1
        m[hit] = rng.integers(0, 20, size=int(hit.sum()))
        for at in (36, 24, 12):                                       # inserts of 0 .. 4 residues at the same three positions
            width = (k // {36: 1, 24: 5, 12: 25}[at]) % 5
            m = np.insert(m, at, rng.integers(0, 20, size=width).astype(np.uint8))
        recs.append(m)
    S = get_blosum62()
    with SeqSet(recs) as ss:
        held = ss.hits(S, DEL, EXT, 100.0, rectangle(0, 1, 1, 300))
        assert len(held) > 256
        res, strs = held.strings()
        widths = {}
        for hit_runs, sx in zip(runs_of(held, res, strs), res["start_x"]):
            for a, n, seen in hit_runs:
                widths.setdefault(int(sx) + seen, set()).add(n)
        assert sum(len(v) >= 3 for v in widths.values()) >= 2, "runs of several lengths meet at the same positions"
        label = np.zeros(301, dtype=np.uint32)
        got, (mats, lists, recs_w, summ), _ = check(held, label)
        assert int(got.records["rows"][0]) == len(held) > 256 and got.hits(0).tolist() == list(range(len(held)))
        again = held.msa(label)
        assert again.out.tobytes() == got.out.tobytes() and again.row_hit.tobytes() == got.row_hit.tobytes()
        assert again.records.tobytes() == got.records.tobytes() and again.summary == got.summary


# ---------------------------------------------------------------- the families of a small protein set
@pytest.fixture(scope="module")
def families():
    S = get_blosum62()
    codes, family = cluster_cases.family_set()
    with SeqSet(codes) as ss:
        labels = ss.hits(S, 11, 2, F_MIN, None).cluster(mode="greedy").label.copy()
        yield ss, codes, S, labels, family


def test_who_contributes(families):
    ss, codes, S, labels, family = families
    n = len(ss)
    held = ss.hits(S, 11, 2, F_MIN, rectangle(0, n, 0, n))               # the full square: every pair in both orientations, the self pairs
    reps = profile.default_centers(labels)
    assert len(reps) >= 3
    full, (mats, lists, recs, summ), (res, strs, seqs) = check(held, labels)
    assert summ["self_pairs"] > 0 and summ["between_members"] > 0 and summ["unlisted"] == 0 and summ["contributing"] > 0
    assert any(centre_runs(s[0], len(s[0]) - 1) for s in strs) and any(centre_runs(s[1], len(s[1]) - 1) for s in strs), "gaps occur"
    assert any(r[3] > 0 for r in recs)
    pairs = {(int(a), int(b)) for a, b in zip(held.q, held.t)}
    for rows, (c, n_rows, _w, _i) in zip(lists, recs):                  # both orientations contribute, each a row of its own
        others = [int(held.t[h]) if int(held.q[h]) == c else int(held.q[h]) for h in rows[1:]]
        assert n_rows % 2 == 0 and all(others.count(m) == 2 and (c, m) in pairs and (m, c) in pairs for m in set(others))
    upper, (_m, _l, half, half_summ), _ = check(ss.hits(S, 11, 2, F_MIN, None), labels)
    held = ss.hits(S, 11, 2, F_MIN, rectangle(0, n, 0, n))
    assert [r[1] for r in recs] == [2 * r[1] for r in half] and half_summ["self_pairs"] == 0
    # a label NONE: the family struck out contributes nowhere; its self pairs still count
    lab = labels.copy()
    lab[labels == reps[0]] = R.NONE
    got, (_m, _l, _r, s2), _ = check(held, lab)
    assert got.centers.tolist() == reps[1:].tolist() and s2["self_pairs"] == summ["self_pairs"] and s2["contributing"] < summ["contributing"]
    # an unlisted centre
    two, (_m, _l, _r, s3), _ = check(held, labels, centers=reps[:2])
    assert s3["unlisted"] == summ["contributing"] - s3["contributing"] > 0 and s3["between_members"] == summ["between_members"]
    assert two.rows(1).tolist() == full.rows(1).tolist()
    # no centre at all, and listed centres without a hit: a loner and a member
    none, (_m, _l, _r, s4), _ = check(held, labels, centers=np.zeros(0, dtype=np.uint32))
    assert len(none.out) == 0 and len(none.row_hit) == 0 and s4["unlisted"] == summ["contributing"]
    sizes = np.bincount(labels[labels != R.NONE].astype(np.int64), minlength=n)
    loner = int(np.flatnonzero(sizes == 1)[0])
    member = int(np.flatnonzero((labels == reps[0]) & (np.arange(n) != reps[0]))[0])
    listed = np.unique(np.array([loner, member, int(reps[0])], dtype=np.uint32))
    got, _w, _ = check(held, labels, centers=listed)
    for i, c in enumerate(listed.tolist()):
        if c != int(reps[0]):
            assert got.rows(i).tolist() == [codes[c].tolist()] and int(got.records["inserted"][i]) == 0
    # a filter that drops some hits, and one that keeps all
    kept = held.filter(S, **FILTER)
    assert 0 < len(kept) < len(held)
    _g, (_m, _l, _r, s5), _ = check(held, labels, matrix=S, **FILTER)
    assert 0 < s5["contributing"] < summ["contributing"]
    everything, (_m, _l, _r, s6), _ = check(held, labels, matrix=S)
    assert everything.out.tobytes() == full.out.tobytes() and s6 == summ


def test_after_every_kind_of_held_pass(families):
    ss, codes, S, labels, family = families
    n = len(ss)
    for mode in ("greedy", "components"):
        held = ss.hits(S, 11, 2, F_MIN, None)
        clusters = held.cluster(mode=mode)
        got, (_m, _l, _r, summ), _ = check(held, clusters)
        assert got.centers.tolist() == [int(r["label"]) for r in clusters.records if r["size"] >= 2] and summ["contributing"] > 0
    best = ss.best(S, 11, 2, 3, skip_self=True)
    got, (_m, _l, _r, summ), _ = check(best, best.cluster(mode="greedy"))
    assert summ["contributing"] > 0 and len(got) >= 3
    cand = ss.prefilter(3, 20, min_shared=0, min_per_1024=128, block=rectangle(0, n, 0, n))
    assert 0 < len(cand) < n * n
    held = cand.hits(S, 11, 2, F_MIN)
    got, (_m, _l, _r, summ), _ = check(held, labels)
    assert summ["contributing"] > 0 and summ["self_pairs"] > 0
    held = cand.best(S, 11, 2, 4, skip_self=True)
    got, (_m, _l, _r, summ), _ = check(held, held.cluster(mode="greedy"), matrix=S, min_identity=0.3)
    assert summ["contributing"] > 0
    text = got.text(0)
    assert len(text) == int(got.records["rows"][0]) + 1 and text[0].replace("-", "") == Protein.vec_to_str(codes[int(got.centers[0])])


# ---------------------------------------------------------------- the held state, the refusals
def digest(held, S, labels):
    lst = held.__class__(held.owner, len(held), held.semantics)       # (held_list again)
    res, strs = held.strings()
    h = hashlib.sha256()
    for part in (lst.index, lst.q, lst.t, lst.f, res, held.report(S), held.profiles(labels).out):
        h.update(part.tobytes())
    for x, y in strs:
        h.update(x.tobytes())
        h.update(y.tobytes())
    return h.hexdigest()


def test_state_and_refusals(families):
    ss, codes, S, labels, family = families
    lib = ss.lib
    held = ss.hits(S, 11, 2, F_MIN, None)
    before = digest(held, S, labels)
    s0 = ss.stats()
    first = held.msa(labels, matrix=S, **FILTER)
    s1 = ss.stats()
    assert (s1["fill_ms"], s1["refill_ms"]) == (s0["fill_ms"], s0["refill_ms"]) and s1["fetch_kernel_ms"] > 0 and s1["wall_ms"] >= s1["fetch_kernel_ms"]
    assert digest(held, S, labels) == before
    plain = held.msa(labels)
    assert digest(held, S, labels) == before
    INV, UNS = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED
    lab = np.ascontiguousarray(labels, dtype=np.uint32)
    cen = profile.default_centers(labels)
    rec = np.full(16 * len(cen), 7, dtype=np.uint8)
    summ = _ffi.MsaSummary(9, 9, 9, 9, 9, 9, 9, 9)
    p, _alive = runtime.make_params(_ffi.CORE_LOCAL, 0.0, 0.0, S)
    flt = _ffi.HitFilter(FILTER["min_identity"], FILTER["min_q_cover"], 0.0, 0, 0)

    def plan(params=None, flags=0, f=None, label=lab, centers=cen, n_centers=None, r=rec, s=summ):
        return lib.aln_seqset_held_msa_plan(ss.handle, C.byref(params) if params is not None else None, flags, C.byref(f) if f is not None else None,
                                            label.ctypes.data if label is not None else None, centers.ctypes.data if centers is not None else None,
                                            len(centers) if n_centers is None else n_centers, r.ctypes.data if r is not None else None,
                                            C.byref(s) if s is not None else None)

    total, rows = plain.summary["bytes"], plain.summary["total_rows"]
    out = np.full(total + 8, 7, dtype=np.uint8)
    row_hit = np.full(rows + 2, 7, dtype=np.uint32)

    def fill(o=out, cap=total, r=row_hit, cap_rows=rows):
        return lib.aln_seqset_held_msa_fill(ss.handle, o.ctypes.data if o is not None else None, cap, r.ctypes.data if r is not None else None, cap_rows)

    # the plan's refusals leave the records, the summary, the stats and the plan before them as they were
    stats = ss.stats()
    pwm = _ffi.Params.from_buffer_copy(bytes(p))
    pwm.semantics = _ffi.PWM_LOCAL
    assert plan(flags=1) == INV and plan(flags=2, params=p, f=flt) == INV
    assert plan(label=None) == INV and plan(centers=None, n_centers=len(cen)) == INV and plan(r=None) == INV and plan(s=None) == INV
    assert plan(centers=cen[::-1].copy()) == INV and plan(centers=np.array([0, len(ss)], dtype=np.uint32)) == INV
    assert plan(params=p) == INV and plan(f=flt) == INV and plan(params=p, f=_ffi.HitFilter(0.0, 0.0, 0.0, 0, 1)) == INV
    assert plan(params=pwm, f=flt) == UNS
    assert (rec == 7).all() and [getattr(summ, f[0]) for f in _ffi.MsaSummary._fields_] == [9] * 8 and ss.stats() == stats
    # the fill's: a capacity one byte or one row short, null buffers
    assert fill(cap=total - 1) == INV and fill(cap_rows=rows - 1) == INV and fill(o=None) == INV and fill(r=None) == INV
    assert (out == 7).all() and (row_hit == 7).all() and ss.stats() == stats
    assert fill() == 0 and out[:total].tobytes() == plain.out.tobytes() and row_hit[:rows].tolist() == plain.row_hit.tolist()
    assert (out[total:] == 7).all() and (row_hit[rows:] == 7).all()
    assert fill(cap=total + 8, cap_rows=rows + 2) == 0 and (out[total:] == 7).all()          # the same plan again, more room than it needs
    assert plan(params=p, f=flt) == 0 and summ.held == len(held) and summ.bytes == first.summary["bytes"]
    assert digest(held, S, labels) == before
    # a new held pass: the plan is of hits that are gone
    ss.hits(S, 11, 2, F_MIN, None)
    out.fill(7)
    row_hit.fill(7)
    assert fill(cap=total + 8, cap_rows=rows + 2) == INV and b"plan" in lib.aln_last_error() and (out == 7).all() and (row_hit == 7).all()
    assert plan() == 0 and fill() == 0 and out[:total].tobytes() == plain.out.tobytes()
    # no held pass at all: a score pass replaces it
    ss.score(S, 11, 2, rectangle(0, 2, 0, 2))
    out.fill(7)
    assert plan() == INV and fill() == INV and (out == 7).all()


# ---------------------------------------------------------------- the C99 caller, and the command
def hexd(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def test_through_c(families, tmp_path):
    """tests/abi_msa.c: both exports called from C99 on buffers of exactly the documented sizes, each followed by a guard zone"""
    ss, codes, S, labels, family = families
    n = len(ss)
    cen = profile.default_centers(labels)
    words = [len(codes)] + [len(c) for c in codes] + [int(x) for c in codes for x in c]
    words += [S.shape[0], S.shape[1]] + [hexd(x) for x in S.ravel()] + [hexd(11.0), hexd(2.0), hexd(F_MIN), BLANK, hexd(FILTER["min_identity"]), hexd(FILTER["min_q_cover"])]
    words += [int(x) for x in labels] + [len(cen)] + [int(x) for x in cen]
    case = tmp_path / "case.txt"
    case.write_text(" ".join(str(w) for w in words) + "\n")
    exe = native_build.build_msa_harness()
    run = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr
    lines = [l.split() for l in run.stdout.splitlines()]
    assert lines[-1] == ["guards", "ok"]
    held = ss.hits(S, 11, 2, F_MIN, rectangle(0, n, 0, n))
    assert ["held", str(len(held))] in lines
    calls = [k for k, l in enumerate(lines) if l[:2] == ["rc", "held_msa_plan"]]
    assert [lines[k][2:] for k in calls] == [["0", "0"], ["1", "0"]]
    for k, th in zip(calls, (None, FILTER)):
        kept = held.filter(S, **th) if th else None
        mats, lists, recs, summ, _ = R.from_held(held, labels, cen, BLANK, kept)
        want_out, want_rows = R.flat(mats, lists)
        rec_line, sum_line, fill_line, rows_line, out_line = lines[k + 1:k + 6]
        assert (rec_line[0], sum_line[0], rows_line[0], out_line[0]) == ("records", "summary", "row_hit", "out")
        assert fill_line == ["rc", "held_msa_fill", "1" if th else "0", "0"]
        flat = [int(x) for x in rec_line[1:]]
        assert [tuple(flat[i:i + 4]) for i in range(0, len(flat), 4)] == recs
        assert [int(x) for x in sum_line[1:]] == [summ[key] for key in R.SUMMARY_KEYS]
        assert [int(x) for x in rows_line[1:]] == want_rows.tolist() and [int(x) for x in out_line[1:]] == want_out.tolist()
        assert summ["contributing"] > 0


def test_the_command(capsys, tmp_path):
    path = os.path.join(ROOT, "tests", "golden", "protein.fasta")
    records = read_fasta(path)
    heads = [r.head.decode("utf-8", "replace") for r in records]
    codes = encode_records(records, Protein)
    S = get_blosum62()
    out = str(tmp_path / "families.fa")
    argv = ["-i", path, "--f-min", "30", "--cluster", "greedy", "--min-identity", "0.3"]
    assert allpairs.main(argv + ["--msa", out]) == 0
    with_file = capsys.readouterr().out
    assert allpairs.main(argv) == 0
    assert capsys.readouterr().out == with_file                         # the rows of --cluster are what they were
    blocks = [b.splitlines() for b in open(out).read().split("\n\n") if b.strip()]
    assert open(out).read().endswith("\n\n")
    with SeqSet(codes) as ss:
        held = ss.hits(S, 11.0, 2.0, 30.0, None)
        clusters = held.cluster(S, mode="greedy", min_identity=0.3)
        kept = held.filter(S, min_identity=0.3)
        cen = profile.default_centers(clusters.label)
        mats, lists, recs, summ, _ = R.from_held(held, clusters.label, cen, BLANK, kept)
        assert len(blocks) == len(mats) >= 1 and summ["contributing"] > 0
        for block, m, rows, (c, n_rows, width, _i) in zip(blocks, mats, lists, recs):
            assert len(block) == 2 * (n_rows + 1) and n_rows >= 1
            names, texts = block[0::2], block[1::2]
            members = [int(held.t[h]) if int(held.q[h]) == c else int(held.q[h]) for h in rows[1:]]
            assert names == [">" + heads[c]] + [">%s hit=%d" % (heads[mem], h) for mem, h in zip(members, rows[1:])]
            assert all(len(t) == width for t in texts)
            # parsed back: the letters are the codes, `-` is the blank
            back = [[BLANK if ch == "-" else int(Protein.str_to_vec(ch)[0]) for ch in t] for t in texts]
            assert back == m.tolist()
