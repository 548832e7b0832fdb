"""Profiles on the device (aln_seqset_held_profiles, HeldHits.profiles) against the plain Python rule of profile_ref.py fed from
held.strings() and the held list: every element, record and counter, integer for integer, and the position rule's premise (a centre's
aligned residues are the set's residues at the positions the rule assigns) asserted on the way.

A held entry with a status other than ALN_OK cannot be produced through the public calls (failed pairs are never hits, and the re-fill
runs pairs that succeeded): the tests assert that every held status is ALN_OK; that branch of the rule is profile_ref's and one line
of the kernel."""
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
import profile_ref as R  # noqa: E402
from aligner_amd import _ffi, allpairs, cluster, profile, runtime  # noqa: E402
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


def check(held, labels, centers=None, n_codes=None, matrix=None, skip_seed=True, **th):
    """HeldHits.profiles against the reference over held.strings(); returns (Profiles, the reference's summary)"""
    ss = held.owner
    got = held.profiles(labels, centers=centers, n_codes=n_codes, matrix=matrix, skip_seed=skip_seed, **th)
    up_down = ss.stats()
    kept = held.filter(matrix, skip_seed=skip_seed, **th) if matrix is not None else None
    lab = profile.labels_of(labels)
    want_out, want_rec, want_sum = R.from_held(held, lab, got.centers, got.n_codes, BLANK, skip_seed, kept)
    assert got.out.dtype == np.uint32 and got.out.tolist() == want_out.tolist()
    assert [tuple(int(x) for x in r) for r in got.records.tolist()] == want_rec
    assert got.summary == want_sum and got.summary["overflow"] == 0
    # the sizing helper and the layout against numpy
    total = C.c_uint64(0)
    cen = got.centers
    assert ss.lib.aln_seqset_profile_elements(ss.handle, cen.ctypes.data if len(cen) else None, len(cen), got.n_codes, C.byref(total)) == 0
    assert total.value == got.summary["elements"] == len(got.out) == int(((got.n_codes + 2) * ss.len[cen.astype(np.int64)]).sum())
    for i in range(len(got)):
        view = got.counts(i)
        assert view.shape == (got.n_codes + 2, int(ss.len[cen[i]]))
        assert int(view[:got.n_codes].sum()) == int(got.records["matched"][i]) and int(view[got.n_codes].sum()) == int(got.records["deleted"][i])
    bits = 4 * ((matrix.size + 31) // 32) if matrix is not None and len(held) else 0
    assert up_down["bytes_up"] == 8 * len(held) + 4 * len(ss) + 12 * len(cen) + bits
    assert up_down["bytes_down"] == 4 * len(got.out) + 16 * len(cen) + 64
    return got, want_sum


# ---------------------------------------------------------------- wave rounds: a hand-built family around the 64-column rounds
def wave_set():
    rng = np.random.default_rng(64)
    centre = rng.integers(0, 20, size=134).astype(np.uint8)
    recs = [centre]
    for a in (62, 63, 64, 65, 66):                                   # a deletion, an insertion, both, around columns 62 .. 66 and 126 .. 130
        b = a + 64
        recs.append(np.delete(centre, np.arange(a, a + 4)))
        recs.append(np.insert(centre, a, rng.integers(0, 20, size=3).astype(np.uint8)))
        recs.append(np.delete(centre, np.arange(b, b + 3)))
        recs.append(np.insert(centre, b, rng.integers(0, 20, size=4).astype(np.uint8)))
        recs.append(np.insert(np.delete(centre, np.arange(b, b + 4)), a, rng.integers(0, 20, size=2).astype(np.uint8)))
        recs.append(np.insert(np.delete(centre, np.arange(a, a + 5)), b - 5, rng.integers(0, 20, size=5).astype(np.uint8)))
    recs.append(np.insert(centre[:120], 20, rng.integers(0, 20, size=3).astype(np.uint8)))      # an insertion in front of column 64
    for w in (61, 62, 63, 64, 65, 66, 67):                           # exact pieces: that many aligned columns and the seed
        recs.append(centre[9:9 + w].copy())
    recs.append(rng.integers(0, 20, size=90).astype(np.uint8))       # an unrelated record
    assert 38 <= len(recs) <= 42 and all(60 <= len(r) <= 140 for r in recs)
    return recs


@pytest.fixture(scope="module")
def waves():
    S = get_blosum62()
    with SeqSet(wave_set()) as ss:
        yield ss, S


@pytest.mark.parametrize("skip_seed", [True, False])
def test_wave_rounds(waves, skip_seed):
    ss, S = waves
    n = len(ss)
    held = ss.hits(S, 11, 2, 200.0, None)
    res, strs = held.strings()
    assert (res["status"] == 0).all()
    label = np.zeros(n, dtype=np.uint32)
    label[n - 1] = n - 1
    # coverage, from the strings: the hits of the centre (the query of every one: record 0 of an upper block)
    mine = np.flatnonzero(held.q == 0)
    assert len(mine) >= 35 and (held.t[mine] != 0).all()
    counted = [R.counted_columns(int(res["aln_len"][h]), 1 if skip_seed else 0) for h in mine]
    assert max(counted) > 128
    assert {63, 64, 65} <= set(counted)
    blanks = [np.flatnonzero(strs[h][0][:c] == BLANK) for h, c in zip(mine, counted)]
    assert any(len(b) and b.max() >= 64 for b in blanks) and any(len(b) and b.min() < 64 for b in blanks)
    assert any(len(b) and b.max() >= 128 for b in blanks)
    assert any((strs[h][1][:c] == BLANK)[60:68].any() for h, c in zip(mine, counted))           # deletions across the first round's edge
    got, summ = check(held, label, skip_seed=skip_seed)
    assert got.centers.tolist() == [0] and summ["contributing"] == len(mine) and summ["between_members"] == len(held) - len(mine) > 100
    assert int(got.records["deleted"][0]) > 50
    if not skip_seed:
        assert int(got.counts(0).sum()) == int(check(held, label, skip_seed=True)[0].counts(0).sum()) + len(mine)


# ---------------------------------------------------------------- the families of a small protein set
@pytest.fixture(scope="module")
def families():
    S = get_blosum62()
    codes, family = cluster_cases.family_set()
    with SeqSet(codes) as ss:
        labels = ss.hits(S, 11, 2, F_MIN, None).cluster(mode="greedy").label.copy()
        yield ss, codes, S, labels, family


def test_orientation_the_full_square(families):
    ss, codes, S, labels, family = families
    n = len(ss)
    held = ss.hits(S, 11, 2, F_MIN, rectangle(0, n, 0, n))
    got, summ = check(held, labels)
    check(held, labels, skip_seed=False)                                       # with the seed column counted
    assert len(got) >= 3
    # the centre is the query of one listing and the target of the other: both count
    upper = ss.hits(S, 11, 2, F_MIN, None)
    half, half_summ = check(upper, labels)
    assert got.records["hits"].tolist() == (2 * half.records["hits"]).tolist() and summ["contributing"] == 2 * half_summ["contributing"] > 0
    assert summ["self_pairs"] > 0 and half_summ["self_pairs"] == 0              # (every record long enough hits itself)
    c = int(got.centers[0])
    as_q = ss.hits(S, 11, 2, F_MIN, rectangle(c, 1, 0, n))                     # one against many: the centre as the query ...
    a, _s = check(as_q, labels)
    as_t = ss.hits(S, 11, 2, F_MIN, rectangle(0, n, c, 1))                     # ... and as the target
    b, _s = check(as_t, labels)
    assert a.records["hits"][0] == b.records["hits"][0] == half.records["hits"][0] > 0
    assert (a.counts(0) + b.counts(0)).tolist() == got.counts(0).tolist()


@pytest.mark.parametrize("name", ["core_local", "core_global", "real_valued"])
def test_schemes(families, name):
    ss, codes, S, labels, family = families
    sem, m, d, e = {"core_local": (_ffi.CORE_LOCAL, S, 11.0, 2.0), "core_global": (_ffi.CORE_GLOBAL, S, 4.0, 4.0),
                    "real_valued": (_ffi.CORE_LOCAL, S * 0.37 + 0.013, 11.3, 2.1)}[name]      # (the schemes of tests/test_seqset_gpu.py)
    if sem == _ffi.CORE_GLOBAL:
        # every pair of a small square is a hit (f is 0.0); a labelling of the caller's: the first record of every ancestor
        first = {}
        lab = np.array([first.setdefault(a, i) if a >= 0 else R.NONE for i, a in enumerate(family)], dtype=np.uint32)
        lab[16:] = R.NONE
        held = ss.hits(m, d, e, 0.0, rectangle(0, 16, 0, 16), semantics=sem)
        assert len(held) == 256
        for skip_seed in (True, False):
            got, summ = check(held, lab, skip_seed=skip_seed)
            assert summ["contributing"] > 0 and summ["between_members"] > 0 and summ["self_pairs"] == 16           # (a self pair is one whatever its label)
            for i in range(len(got)):                                          # a global alignment covers the whole centre
                depth = got.counts(i).sum(axis=0)
                assert depth.min() >= got.records["hits"][i] > 0 and (skip_seed is False or depth.max() == depth.min())
    else:
        held = ss.hits(m, d, e, F_MIN * (0.37 if name == "real_valued" else 1.0), None, semantics=sem)
        got, summ = check(held, labels)
        assert summ["contributing"] > 5
        check(held, labels, matrix=m, **FILTER)


def test_who_counts(families):
    ss, codes, S, labels, family = families
    n = len(ss)
    held = ss.hits(S, 11, 2, F_MIN, rectangle(0, n, 0, n))
    assert (held.strings()[0]["status"] == 0).all()
    reps = profile.default_centers(labels)
    assert len(reps) >= 3
    sizes = np.bincount(labels[labels != R.NONE].astype(np.int64), minlength=n)
    assert (sizes[reps] >= 3).any()                                            # a family with member - member hits
    full, summ = check(held, labels)
    assert summ["between_members"] > 0 and summ["unlisted"] == 0 and summ["self_pairs"] > 0
    # labels with NONE: a family struck out counts nowhere, its self pairs still do
    lab = labels.copy()
    lab[labels == reps[0]] = R.NONE
    got, s2 = check(held, lab)
    assert got.centers.tolist() == reps[1:].tolist() and s2["self_pairs"] == summ["self_pairs"] and s2["contributing"] < summ["contributing"]
    # two families only; a centre left out of `centers`: its hits are unlisted
    two, s3 = check(held, labels, centers=reps[:2])
    assert s3["unlisted"] == summ["contributing"] - s3["contributing"] > 0
    assert s3["between_members"] == summ["between_members"] and s3["self_pairs"] == summ["self_pairs"]
    assert two.counts(1).tolist() == full.counts(1).tolist()
    # no centre at all, and a listed centre without hits: a loner, and a member (never the centre of a hit)
    none, s4 = check(held, labels, centers=np.zeros(0, dtype=np.uint32))
    assert len(none.out) == 0 and s4["unlisted"] == summ["contributing"] and s4["contributing"] == 0
    loner = int(np.flatnonzero(sizes == 1)[0])
    member = int(np.flatnonzero((labels == reps[0]) & (np.arange(n) != reps[0]))[0])
    listed = np.unique(np.array([loner, member, int(reps[0])], dtype=np.uint32))
    got, s5 = check(held, labels, centers=listed)
    for i, c in enumerate(listed.tolist()):
        if c != int(reps[0]):
            assert int(got.records["hits"][i]) == 0 and not got.counts(i).any()
    # a labelling that names no sequence of the set: every hit with both ends in it lies between members
    far = np.full(n, 0xFFFFFFF0, dtype=np.uint32)
    got, s6 = check(held, far, centers=reps)
    assert s6["contributing"] == 0 and s6["between_members"] == len(held) - s6["self_pairs"] and not got.out.any()
    # fewer and more codes with a row of their own
    small, _s = check(held, labels, n_codes=4)
    assert small.counts(0)[5].sum() > 0                                        # codes 4 .. 19 fall into the last row
    wide, _s = check(held, labels, n_codes=64)
    assert wide.counts(0)[:20].tolist() == full.counts(0)[:20].tolist() and not wide.counts(0)[20:64].any()


def test_with_a_filter(families):
    ss, codes, S, labels, family = families
    n = len(ss)
    held = ss.hits(S, 11, 2, F_MIN, rectangle(0, n, 0, n))
    plain, s0 = check(held, labels)
    kept = held.filter(S, **FILTER)
    assert 0 < len(kept) < len(held)
    got, s1 = check(held, labels, matrix=S, **FILTER)
    assert 0 < s1["contributing"] < s0["contributing"] and s1["self_pairs"] == s0["self_pairs"]
    check(held, labels, matrix=S, skip_seed=False, min_identity=0.3, min_t_cover=0.6, min_columns=40)
    everything, s2 = check(held, labels, matrix=S)                             # a filter that keeps every hit
    assert everything.out.tolist() == plain.out.tolist() and s2 == s0


def test_labels_of_both_cluster_modes(families):
    ss, codes, S, labels, family = families
    held = ss.hits(S, 11, 2, F_MIN, None)
    for mode in ("greedy", "components"):
        clusters = held.cluster(mode=mode)
        got, summ = check(held, clusters)
        want = [int(r["label"]) for r in clusters.records if r["size"] >= 2]
        assert got.centers.tolist() == want and len(want) >= 3 and summ["contributing"] > 0 and summ["unlisted"] == 0
        f = got.frequency(0)
        own = codes[want[0]]
        v = Protein.volume()                                               # the default n_codes
        assert got.n_codes == v and f.shape == (v, len(own)) and f.dtype == np.float64
        assert (f[own, np.arange(len(own))] >= 1.0).all() and f.sum() == got.counts(0)[:v].sum() + len(own)
    filtered = held.cluster(S, mode="greedy", **FILTER)
    check(held, filtered, matrix=S, **FILTER)


def test_contention():
    """300 members against one centre of 70 residues: every column of the profile takes up to 300 adds"""
    rng = np.random.default_rng(300)
    centre = rng.integers(0, 20, size=70).astype(np.uint8)
    recs = [centre]
    for k in range(300):
        m = centre.copy()
        hit = rng.random(70) < 0.15
        m[hit] = rng.integers(0, 20, size=int(hit.sum()))
        if k % 3 == 0:
            m = np.delete(m, np.arange(20 + k % 30, 23 + k % 30))
        if k % 5 == 0:
            m = m[k % 7:]
        recs.append(m)
    S = get_blosum62()
    with SeqSet(recs) as ss:
        held = ss.hits(S, 11, 2, 100.0, rectangle(0, 1, 1, 300))
        assert len(held) >= 295
        res, strs = held.strings()
        depth = np.zeros(70, dtype=np.int64)                          # from the summaries and strings: who covers which position
        for r, (qs, ts) in zip(res, strs):
            covered = int((qs[:int(r["aln_len"]) - 1] != BLANK).sum())
            depth[int(r["start_x"]):int(r["start_x"]) + covered] += 1
        got, summ = check(held, np.zeros(301, dtype=np.uint32))
        assert got.counts(0).sum(axis=0).tolist() == depth.tolist() and depth.max() >= 295
        assert summ["contributing"] == len(held) == int(got.records["hits"][0]) and int(got.records["deleted"][0]) >= 250


# ---------------------------------------------------------------- the held state, the refusals
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


def answers(held, S):
    pos, rep = held.filter(S, with_reports=True, **FILTER)
    c = held.cluster(S, mode="greedy", **FILTER)
    sig = held.significance_records(S, 11, 2, 7, per_pair=8, keep=np.arange(min(len(held), 6), dtype=np.uint32))[0]
    return (digest(held), held.report(S).tobytes(), pos.tobytes(), rep.tobytes(), c.label.tobytes(), c.records.tobytes(), sig.tobytes())


def test_the_held_state_is_left_as_it_was(families):
    ss, codes, S, labels, family = families
    held = ss.hits(S, 11, 2, F_MIN, None)
    before = answers(held, S)
    s0 = ss.stats()
    first = held.profiles(labels, matrix=S, **FILTER)
    s1 = ss.stats()
    assert (s1["fill_ms"], s1["refill_ms"]) == (s0["fill_ms"], s0["refill_ms"]) and s1["fetch_kernel_ms"] > 0 and s1["wall_ms"] >= s1["fetch_kernel_ms"]
    held.profiles(labels, skip_seed=False, n_codes=7)
    again = held.profiles(labels, matrix=S, **FILTER)
    assert again.out.tobytes() == first.out.tobytes() and again.records.tobytes() == first.records.tobytes() and again.summary == first.summary
    assert answers(held, S) == before


def test_refusals_leave_everything_as_it_was(families):
    ss, codes, S, labels, family = families
    lib = ss.lib
    n = len(ss)
    held = ss.hits(S, 11, 2, F_MIN, None)
    before = digest(held)
    stats = ss.stats()
    p, _alive = runtime.make_params(_ffi.CORE_LOCAL, 0.0, 0.0, S)
    cen = profile.default_centers(labels)
    total = int((22 * ss.len[cen.astype(np.int64)]).sum())
    out = np.full(total, 7, dtype=np.uint32)
    rec = np.full(16 * len(cen), 7, dtype=np.uint8)
    summ = _ffi.ProfileSummary(9, 9, 9, 9, 9, 9, 9, 9)
    flt = _ffi.HitFilter(0.5, 0.0, 0.0, 0, 0)
    INV, UNS = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED
    lab = np.ascontiguousarray(labels, dtype=np.uint32)

    def call(params=p, flags=1, f=flt, label=lab, centers=cen, n_centers=None, n_codes=20, o=out, cap=total, r=rec, s=summ):
        return lib.aln_seqset_held_profiles(ss.handle, C.byref(params) if params is not None else None, flags, C.byref(f) if f is not None else None,
                                            label.ctypes.data if label is not None else None, centers.ctypes.data if centers is not None else None,
                                            len(centers) if n_centers is None else n_centers, n_codes, o.ctypes.data if o is not None else None, cap,
                                            r.ctypes.data if r is not None else None, C.byref(s) if s is not None else None)

    pwm = _ffi.Params.from_buffer_copy(bytes(p))
    pwm.semantics = _ffi.PWM_LOCAL
    no_matrix = _ffi.Params.from_buffer_copy(bytes(p))
    no_matrix.matrix = None
    assert call(label=None) == INV and call(centers=None, n_centers=len(cen)) == INV and call(o=None) == INV and call(r=None) == INV and call(s=None) == INV
    assert call(centers=cen[::-1].copy()) == INV and call(centers=np.array([3, 3], dtype=np.uint32)) == INV
    assert call(centers=np.array([0, n], dtype=np.uint32)) == INV and b"ascending" in lib.aln_last_error()
    assert call(n_codes=0) == INV and call(n_codes=65) == INV and call(n_codes=0xFFFFFFFF) == INV
    assert call(flags=2) == INV and call(flags=3) == INV and call(flags=2, f=None, params=None) == INV
    assert call(cap=total - 1) == INV and call(cap=0) == INV
    assert call(params=None) == INV and call(f=None) == INV                       # a filter without params, params without a filter
    assert call(f=_ffi.HitFilter(0.0, 0.0, 0.0, 0, 1)) == INV and call(params=no_matrix) == INV
    assert call(params=pwm) == UNS
    t = C.c_uint64(9)
    assert lib.aln_seqset_profile_elements(ss.handle, cen.ctypes.data, len(cen), 0, C.byref(t)) == INV
    assert lib.aln_seqset_profile_elements(ss.handle, cen.ctypes.data, len(cen), 20, None) == INV
    assert lib.aln_seqset_profile_elements(ss.handle, cen[::-1].copy().ctypes.data, len(cen), 20, C.byref(t)) == INV and t.value == 9
    assert (out == 7).all() and (rec == 7).all() and [getattr(summ, f[0]) for f in _ffi.ProfileSummary._fields_] == [9] * 8
    assert ss.stats() == stats and digest(held) == before
    assert call() == 0 and summ.reserved == 0 and summ.held == len(held) and summ.elements == total
    assert call(cap=total + 5, f=None, params=None) == 0
    # no held pass: a score pass replaces it; the sizing helper needs none
    ss.score(S, 11, 2, rectangle(0, 2, 0, 2))
    out.fill(7)
    assert call() == INV and call(f=None, params=None) == INV and (out == 7).all()
    assert lib.aln_seqset_profile_elements(ss.handle, cen.ctypes.data, len(cen), 20, C.byref(t)) == 0 and t.value == total


# ---------------------------------------------------------------- the C99 caller, and the command
def hexd(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def test_through_c(families, tmp_path):
    """tests/abi_profile.c: both exports called from C99 on buffers of exactly the documented sizes, each followed by a guard zone"""
    ss, codes, S, labels, family = families
    n = len(ss)
    cen = profile.default_centers(labels)
    words = [len(codes)] + [len(c) for c in codes] + [int(x) for c in codes for x in c]
    words += [S.shape[0], S.shape[1]] + [hexd(x) for x in S.ravel()] + [hexd(11.0), hexd(2.0), hexd(F_MIN), BLANK, hexd(FILTER["min_identity"]), hexd(FILTER["min_q_cover"])]
    words += [int(x) for x in labels] + [len(cen)] + [int(x) for x in cen] + [20]
    case = tmp_path / "case.txt"
    case.write_text(" ".join(str(w) for w in words) + "\n")
    exe = native_build.build_profile_harness()
    run = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr
    lines = [l.split() for l in run.stdout.splitlines()]
    assert lines[-1] == ["guards", "ok"]
    held = ss.hits(S, 11, 2, F_MIN, rectangle(0, n, 0, n))
    assert ["held", str(len(held))] in lines
    calls = [k for k, l in enumerate(lines) if l[:2] == ["rc", "held_profiles"]]
    assert [lines[k][2:] for k in calls] == [["0", "0"], ["1", "0"]]
    for k, th in zip(calls, (None, FILTER)):
        py = held.profiles(labels, n_codes=20, matrix=S if th else None, **(th or {}))
        kept = held.filter(S, **th) if th else None
        want_out, want_rec, want_sum = R.from_held(held, labels, cen, 20, BLANK, True, kept)
        out_line, rec_line, sum_line = lines[k + 1], lines[k + 2], lines[k + 3]
        assert (out_line[0], rec_line[0], sum_line[0]) == ("out", "records", "summary")
        assert [int(x) for x in out_line[1:]] == want_out.tolist() == py.out.tolist()
        flat = [int(x) for x in rec_line[1:]]
        assert [tuple(flat[i:i + 4]) for i in range(0, len(flat), 4)] == want_rec
        assert [int(x) for x in sum_line[1:]] == [want_sum[key] for key in R.SUMMARY_KEYS] + [0]
    assert ["elements", str(len(want_out))] in lines


def test_the_command(capsys, tmp_path):
    path = os.path.join(ROOT, "tests", "golden", "protein.fasta")
    records = read_fasta(path)
    heads = [r.head.decode("utf-8", "replace") for r in records]
    codes = encode_records(records, Protein)
    S = get_blosum62()

    def blocks(prof):
        rows = []
        for i, r in enumerate(prof.records):
            rows.append(">%s hits=%d" % (heads[int(r["center"])], int(r["hits"])))
            rows += [",".join(str(int(x)) for x in prof.counts(i)[:, pos]) for pos in range(prof.counts(i).shape[1])]
        return rows

    with SeqSet(codes) as ss:
        hits = ss.hits(S, 11.0, 2.0, 30.0, None)
        got = hits.cluster(mode="components")
        want_components, _s = check(hits, got)
        want_components = blocks(want_components)
        got = hits.cluster(S, mode="greedy", min_identity=0.3)
        want_greedy = blocks(check(hits, got, matrix=S, min_identity=0.3)[0])
        best = ss.best(S, 11.0, 2.0, 3, skip_self=True)
        want_best = blocks(check(best, best.cluster(mode="greedy"))[0])
    assert len(want_components) > 50 and want_components[0].startswith(">")
    assert all(len(row.split(",")) == Protein.volume() + 2 for row in want_components if not row.startswith(">"))

    def run(argv, name):
        out = str(tmp_path / name)
        assert allpairs.main(["-i", path] + argv + ["--profiles", out]) == 0
        with_file = capsys.readouterr().out
        assert allpairs.main(["-i", path] + argv) == 0
        assert capsys.readouterr().out == with_file                     # the rows of --cluster are what they were
        return open(out).read().splitlines()

    assert run(["--f-min", "30", "--cluster", "components"], "a.txt") == want_components
    assert run(["--f-min", "30", "--cluster", "greedy", "--min-identity", "0.3"], "b.txt") == want_greedy
    assert run(["--best", "3", "--cluster", "greedy"], "c.txt") == want_best
