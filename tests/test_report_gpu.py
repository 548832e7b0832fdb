"""Reports of a sequence set's held hits (aln_seqset_held_report / aln_seqset_held_filter, HeldHits.report / filter): the records
field for field against the numpy restatement of the rule (report_ref.py) applied to the CPU oracle's aligned strings and to
held.strings(), at the lengths and seams the wave-per-hit kernel can go wrong at; lists in any order; a scheme other than the held
pass's; the filter across the selection's tile edge and at every capacity; the held state before and after; the refusals; the
command.  tests/test_report_rules_cpu.py shows that the constructed cases are what they claim to be."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle  # noqa: E402
import report_ref  # noqa: E402
from aligner_amd import _ffi, allpairs, runtime  # noqa: E402
from aligner_amd.enums import Protein  # noqa: E402
from aligner_amd.fasta import encode_records, read_fasta  # noqa: E402
from aligner_amd.matrices import get_blosum62  # noqa: E402
from aligner_amd.seqset import REPORT_DTYPE, BestHits, SeqSet, rectangle, report_fractions  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIP = report_ref.SKIP_SEED
NINF = float("-inf")


def same(got, want):
    assert got.dtype == REPORT_DTYPE and len(got) == len(want)
    for name in REPORT_DTYPE.names:
        assert got[name].tolist() == want[name].tolist(), name


def oracle_strings(codes, sem, q, t, S):
    out = []
    for a, b in zip(q, t):
        o = oracle.align(sem, codes[int(a)], codes[int(b)], 11, 2, S)
        assert o["status"] == 0
        out.append((o["qa"], o["ta"]))
    return out


# ---------------------------------------------------------------- the small set: lengths, seams, lists, another scheme
@pytest.fixture(scope="module")
def small():
    oracle.build()
    S = get_blosum62()
    seqs, where = report_ref.small_set(S)
    codes = [Protein.str_to_vec(s) for s in seqs]
    with SeqSet(codes) as ss:
        yield ss, codes, where, S


def hold_local(ss, S):
    """core local, f_min = -inf: every pair that has an alignment"""
    return ss.hits(S, 11, 2, NINF, None, semantics=_ffi.CORE_LOCAL)


@pytest.fixture(scope="module")
def local_ref(small):
    """(q, t, the oracle's strings) of the pairs hold_local holds, computed once"""
    ss, codes, where, S = small
    held = hold_local(ss, S)
    return held.q.copy(), held.t.copy(), oracle_strings(codes, oracle.CORE_LOCAL, held.q, held.t, S)


@pytest.fixture
def local_held(small, local_ref):
    """a fresh held pass (another test's pass has replaced the last one) and the oracle's strings of its pairs"""
    ss, codes, where, S = small
    held = hold_local(ss, S)
    assert held.q.tolist() == local_ref[0].tolist() and held.t.tolist() == local_ref[1].tolist()
    return held, local_ref[2]


def position(held, pair):
    at = np.flatnonzero((held.q == pair[0]) & (held.t == pair[1]))
    assert len(at) == 1
    return int(at[0])


@pytest.mark.parametrize("sem", ["local", "global"])
def test_lengths_and_seam_against_the_oracle(small, sem):
    """every held hit of the small set, both flag values: the model on the oracle's strings, and the model on held.strings()"""
    ss, codes, where, S = small
    if sem == "local":
        held = ss.hits(S, 11, 2, NINF, None, semantics=_ffi.CORE_LOCAL)
        assert 500 < len(held) <= ss.pairs(None)
    else:
        held = ss.hits(S, 11, 2, 0.0, None, semantics=_ffi.CORE_GLOBAL)          # every f is 0: every pair is held
        assert len(held) == ss.pairs(None) and (held.f == 0.0).all()
    ref = oracle_strings(codes, oracle.CORE_LOCAL if sem == "local" else oracle.CORE_GLOBAL, held.q, held.t, S)
    res, own = held.strings()
    assert (res["status"] == 0).all()
    for (a, b), (c, d) in zip(ref, own):
        assert a.tolist() == c.tolist() and b.tolist() == d.tolist()
    for flags in (0, SKIP):
        got = held.report(S, skip_seed=bool(flags))
        same(got, report_ref.reports(ref, S, flags))
        same(got, report_ref.reports(own, S, flags))
    if sem == "local":
        for n in report_ref.LENGTHS:
            h = position(held, where["len%d" % n])
            assert int(res["aln_len"][h]) == n
            r = held.report(S, keep=[h], skip_seed=False)[0]
            assert (int(r["columns"]), int(r["identical"])) == (n, n)
    r = held.report(S, keep=[position(held, where["seam0"]), position(held, where["seam1"])])
    assert (r["t_gap"].tolist(), r["t_gap_open"].tolist(), r["q_gap"].tolist(), r["q_gap_open"].tolist()) == ([10, 0], [1, 0], [0, 3], [0, 1])


def test_lists(local_held, small):
    """1, 3, 4 and 5 entries (four waves per workgroup), reversed, every third position twice: each entry equals the full run's"""
    ss, codes, where, S = small
    held, ref = local_held
    full = held.report(S)
    same(full, report_ref.reports(ref, S, SKIP))
    n = len(held)
    lists = [[n - 1], [7, 0, n - 2], [5, 6, 7, 8], [9, 3, 3, 1, n - 1], list(range(n))[::-1],
             sorted(list(range(n)) + list(range(0, n, 3)))]
    for keep in lists:
        same(held.report(S, keep=keep), full[np.asarray(keep)])
    assert len(held.report(S, keep=[])) == 0


def test_a_failed_entry_and_a_scheme_change(local_held, small):
    """A held entry with a status other than ALN_OK cannot be produced through the public calls: failed pairs are never hits
    (aln_seqset_hits, aln_seqset_best) and the re-fill runs the pairs that succeeded under the same scheme again -- the local pass
    below leaves the pairs without a positive cell out of the held list.  That branch of the rule is the CPU driver's.
    The classes follow the matrix of the report, not the held pass's: a real-valued matrix with 0.0, -0.0 and NaN entries."""
    ss, codes, where, S = small
    held, ref = local_held
    assert len(held) < ss.pairs(None)                                  # (the single-residue sequence has pairs without a positive cell)
    assert (held.strings()[0]["status"] == 0).all()
    rng = np.random.default_rng(3)
    m = np.array([0.0, -0.0, float("nan"), -1.5, 2.25])[rng.integers(0, 5, S.shape)]
    for flags in (0, SKIP):
        got = held.report(m, skip_seed=bool(flags))
        want = report_ref.reports(ref, m, flags)
        same(got, want)
    blosum = held.report(S)
    assert got["positive"].tolist() != blosum["positive"].tolist() and got["identical"].tolist() == blosum["identical"].tolist()
    # a matrix smaller than the residues' codes: a code beyond it is never positive
    tiny = np.zeros((3, 4))
    same(held.report(tiny, keep=np.arange(50)), report_ref.reports(ref[:50], tiny, SKIP))


def test_filter_covers_on_local_hits(local_held, small):
    """local alignments cover their sequences in part: each cover threshold alone and both with an identity, against the model"""
    ss, codes, where, S = small
    held, ref = local_held
    model = report_ref.reports(ref, S, SKIP)
    N, M = ss.len[held.q], ss.len[held.t]
    for th in ((0.0, 0.5, 0.0, 0), (0.0, 0.0, 0.5, 0), (0.0, 1.0, 0.0, 0), (0.0, 0.0, 1.0, 0), (0.3, 0.25, 0.25, 3), (0.0, 0.0, 0.0, 20)):
        want = np.flatnonzero(report_ref.keep(model, N, M, *th))
        assert 0 < len(want) < len(held), th
        assert held.filter(S, *th).tolist() == want.tolist(), th


# ---------------------------------------------------------------- the tile set: the filter
@pytest.fixture(scope="module")
def tile():
    oracle.build()
    S = get_blosum62()
    codes = [Protein.str_to_vec(s) for s in report_ref.tile_set()]
    with SeqSet(codes) as ss:
        yield ss, codes, S


@pytest.fixture(scope="module")
def tile_model(tile):
    """(reports of the model on the oracle's strings, N, M) of every pair of the upper triangle, with and without the seed"""
    ss, codes, S = tile
    n = len(codes)
    q, t = np.triu_indices(n, 1)
    ref = oracle_strings(codes, oracle.CORE_GLOBAL, q, t, S)
    lens = np.array([len(c) for c in codes])
    return {flags: report_ref.reports(ref, S, flags) for flags in (0, SKIP)}, lens[q], lens[t], q, t


def raw_filter(held, S, flags, th, capacity, with_reports=True, fill=0x5A):
    """aln_seqset_held_filter through ctypes: (status, count, positions, reports); the outputs start as `fill` bytes"""
    o = held.owner
    p, _alive = runtime.make_params(held.semantics, 0.0, 0.0, S, outputs=_ffi.OUT_SCORE)
    flt = _ffi.HitFilter(*th, 0)
    pos = np.full(4 * (capacity + 1), fill, dtype=np.uint8).view(np.uint32)
    rep = np.full(40 * (capacity + 1), fill, dtype=np.uint8).view(REPORT_DTYPE)
    count = C.c_uint64(0xDEAD)
    st = o.lib.aln_seqset_held_filter(o.handle, C.byref(p), flags, C.byref(flt), pos.ctypes.data, rep.ctypes.data if with_reports else None,
                                      capacity, C.byref(count))
    return st, int(count.value), pos, rep


FILTERS = {
    "all": (0.0, 0.0, 0.0, 0),
    "all_negative": (NINF, -1.0, -0.0, 0),
    "none_nan_identity": (float("nan"), 0.0, 0.0, 0),
    "none_nan_q": (0.0, float("nan"), 0.0, 0),
    "none_nan_t": (0.0, 0.0, float("nan"), 0),
    "mix": (report_ref.TILE_MIX, 0.0, 0.0, 0),
    "identity": (0.2, 0.0, 0.0, 0),
    # core global with the seed skipped: columns - q_gap == N and columns - t_gap == M for every pair, so a cover threshold alone
    # keeps all at exactly 1.0 and none one ulp above (covers that vary: test_filter_covers_on_local_hits)
    "q_cover_tie": (0.0, 1.0, 0.0, 0),
    "q_cover_above": (0.0, float(np.nextafter(1.0, 2.0)), 0.0, 0),
    "t_cover_tie": (0.0, 0.0, 1.0, 0),
    "t_cover_above": (0.0, 0.0, float(np.nextafter(1.0, 2.0)), 0),
    "columns": (0.0, 0.0, 0.0, 45),
    "together": (0.15, 1.0, 1.0, 40),
}


@pytest.mark.parametrize("held_by", ["hits", "best"])
def test_filter_across_the_tile_edge(tile, tile_model, held_by):
    ss, codes, S = tile
    model, ql, tl, q, t = tile_model
    n = len(codes)
    if held_by == "hits":
        held = ss.hits(S, 11, 2, 0.0, None, semantics=_ffi.CORE_GLOBAL)
        pick = np.arange(len(q))
    else:
        # the k best of an upper-numbered rectangle: rows 0 .. 39 against all, 64 each (every f is 0: the 64 lowest targets)
        held = ss.best(S, 11, 2, 64, block=rectangle(0, 40, 0, n), semantics=_ffi.CORE_GLOBAL)
        assert isinstance(held, BestHits) and len(held) == 40 * 64 > 2048
        pick = None
    assert 2049 <= len(held) <= 4000
    if pick is None:
        ref = oracle_strings(codes, oracle.CORE_GLOBAL, held.q, held.t, S)
        lens = np.array([len(c) for c in codes])
        reps, N, M = {f: report_ref.reports(ref, S, f) for f in (0, SKIP)}, lens[held.q], lens[held.t]
    else:
        assert held.q.tolist() == q.tolist() and held.t.tolist() == t.tolist()
        reps, N, M = model, ql, tl
    for flags in (SKIP, 0):
        same(held.report(S, skip_seed=bool(flags)), reps[flags])
    sizes = {}
    for name, th in FILTERS.items():
        want = np.flatnonzero(report_ref.keep(reps[SKIP], N, M, *th))
        sizes[name] = len(want)
        pos, rep = held.filter(S, *th, with_reports=True)
        assert pos.dtype == np.uint32 and pos.tolist() == want.tolist(), name
        assert held.last_filter_count == len(want)
        same(rep, held.report(S, keep=pos))
        assert held.filter(S, *th).tolist() == want.tolist()
        assert ss.stats()["bytes_down"] == 4 * len(want)
    assert sizes["all"] == sizes["all_negative"] == sizes["q_cover_tie"] == sizes["t_cover_tie"] == len(held)
    assert sizes["none_nan_identity"] == sizes["none_nan_q"] == sizes["none_nan_t"] == sizes["q_cover_above"] == sizes["t_cover_above"] == 0
    for name in ("mix", "identity", "columns", "together"):
        assert 0 < sizes[name] < len(held), (name, sizes[name])
    # without the seed flag the counts are another column's: the filter follows the flag
    want = np.flatnonzero(report_ref.keep(reps[0], N, M, 0.2, 0.0, 0.0, 0))
    assert held.filter(S, 0.2, skip_seed=False).tolist() == want.tolist()
    if held_by == "hits":
        mix = held.filter(S, *FILTERS["mix"])
        assert 2047 in mix and 2048 in mix


def test_filter_capacities(tile, tile_model):
    """capacity 0, the kept count of tile 0, that + 1, total - 1, total: the first `capacity` kept come down, the count is the whole"""
    ss, codes, S = tile
    model, ql, tl, q, t = tile_model
    held = ss.hits(S, 11, 2, 0.0, None, semantics=_ffi.CORE_GLOBAL)
    th = FILTERS["identity"]
    want = np.flatnonzero(report_ref.keep(model[SKIP], ql, tl, *th))
    full = held.report(S)
    in_tile0 = int((want < 2048).sum())
    total = len(want)
    assert 0 < in_tile0 < total - 1
    for cap in (0, in_tile0, in_tile0 + 1, total - 1, total, total + 5):
        for with_reports in (True, False):
            st, count, pos, rep = raw_filter(held, S, SKIP, th, cap, with_reports)
            w = min(cap, total)
            assert st == 0 and count == total
            assert pos[:w].tolist() == want[:w].tolist() and (pos[w:] == 0x5A5A5A5A).all()
            if with_reports:
                same(rep[:w], full[want[:w]])
            assert rep[w if with_reports else 0:].tobytes() == bytes([0x5A]) * (40 * (len(rep) - (w if with_reports else 0)))
            assert ss.stats()["bytes_down"] == (44 if with_reports else 4) * w
    # capacity 0 needs no arrays at all
    o = held.owner
    p, _alive = runtime.make_params(held.semantics, 0.0, 0.0, S, outputs=_ffi.OUT_SCORE)
    count = C.c_uint64(0)
    assert o.lib.aln_seqset_held_filter(o.handle, C.byref(p), SKIP, C.byref(_ffi.HitFilter(*th, 0)), None, None, 0, C.byref(count)) == 0
    assert count.value == total
    pos = held.filter(S, *th, capacity=in_tile0)
    assert pos.tolist() == want[:in_tile0].tolist() and held.last_filter_count == total


# ---------------------------------------------------------------- held state, errors, the command
def test_held_state_survives(small):
    ss, codes, where, S = small
    held = ss.best(S, 11, 2, 5, skip_self=True)
    sample = np.arange(0, len(held), 7, dtype=np.uint32)

    def state():
        lst = held.__class__(ss, len(held), held.semantics)           # (held_list again)
        res, strs = held.strings(sample)
        sig = held.significance_records(S, 11, 2, 9, per_pair=65, keep=[int(np.flatnonzero(ss.len[held.t] >= 6)[0])])[0]
        return (lst.index.tobytes(), lst.q.tobytes(), lst.t.tobytes(), lst.f.tobytes(), res.tobytes(),
                [(a.tobytes(), b.tobytes()) for a, b in strs], sig.tobytes())

    before = state()
    held.strings([0])
    s0 = ss.stats()
    rep = held.report(S)
    s1 = ss.stats()
    assert (s1["fill_ms"], s1["refill_ms"]) == (s0["fill_ms"], s0["refill_ms"])
    assert s1["bytes_down"] == 40 * len(held) and s1["bytes_up"] == 4 * len(held) + 4 * ((S.shape[0] * S.shape[1] + 31) // 32)
    assert s1["fetch_kernel_ms"] >= 0 and s1["wall_ms"] > 0
    held.report(S, keep=[1, 1, 0])
    assert ss.stats()["bytes_down"] == 120
    pos, kept = held.filter(S, min_identity=0.25, with_reports=True)
    s2 = ss.stats()
    assert 0 < len(pos) < len(held)
    assert (s2["fill_ms"], s2["refill_ms"]) == (s0["fill_ms"], s0["refill_ms"])
    assert s2["bytes_down"] == 44 * len(pos) and s2["bytes_up"] == 4 * ((S.shape[0] * S.shape[1] + 31) // 32)
    same(kept, rep[pos])
    assert state() == before
    fr = held.fractions(kept, pos)
    assert fr.tobytes() == report_fractions(kept, ss.len[held.q[pos]], ss.len[held.t[pos]]).tobytes() and (fr["identity"] >= 0.25).all()


def test_refusals_leave_everything_as_it_was(small):
    ss, codes, where, S = small
    lib = ss.lib
    held = ss.hits(S, 11, 2, 40.0, None, semantics=_ffi.CORE_LOCAL)
    n = len(held)
    assert n > 4
    before = held.report(S).tobytes()
    stats = ss.stats()
    p, _alive = runtime.make_params(_ffi.CORE_LOCAL, 0.0, 0.0, S)
    keep = np.array([0, 1], dtype=np.uint32)
    rep = np.full(80, 7, dtype=np.uint8).view(REPORT_DTYPE)
    pos = np.full(2, 7, dtype=np.uint32)
    count = C.c_uint64(77)
    flt = _ffi.HitFilter(0.0, 0.0, 0.0, 0, 0)
    INV, UNS = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED

    def report(params=p, flags=1, k=keep, nk=2, out=rep):
        return lib.aln_seqset_held_report(ss.handle, C.byref(params) if params is not None else None, flags,
                                          k.ctypes.data if k is not None else None, nk, out.ctypes.data if out is not None else None)

    def filt(params=p, flags=1, f=flt, positions=pos, out=rep, cap=2, cnt=count):
        return lib.aln_seqset_held_filter(ss.handle, C.byref(params) if params is not None else None, flags, C.byref(f) if f is not None else None,
                                          positions.ctypes.data if positions is not None else None, out.ctypes.data if out is not None else None, cap,
                                          C.byref(cnt) if cnt is not None else None)

    no_matrix = _ffi.Params.from_buffer_copy(bytes(p))
    no_matrix.matrix = None
    pwm = _ffi.Params.from_buffer_copy(bytes(p))
    pwm.semantics = _ffi.PWM_LOCAL
    big, _alive2 = runtime.make_params(_ffi.CORE_LOCAL, 0.0, 0.0, np.zeros((91, 91)))
    bad_filter = _ffi.HitFilter(0.0, 0.0, 0.0, 0, 1)
    assert report(k=np.array([0, n], dtype=np.uint32)) == INV          # keep[k] >= count
    assert report(k=None) == INV and report(out=None) == INV           # a null pointer with a non-zero length
    assert report(params=None) == INV and report(params=no_matrix) == INV
    assert report(flags=2) == INV and report(flags=3) == INV
    assert report(params=pwm) == UNS and report(params=big) == UNS
    assert report(k=None, nk=0, out=None) == 0                         # nothing listed: nothing asked for
    assert filt(params=None) == INV and filt(params=no_matrix) == INV and filt(f=None) == INV and filt(cnt=None) == INV
    assert filt(positions=None) == INV and filt(flags=4) == INV and filt(f=bad_filter) == INV
    assert filt(params=pwm) == UNS and filt(params=big) == UNS
    assert rep.tobytes() == bytes([7]) * 80 and pos.tolist() == [7, 7] and count.value == 77
    assert ss.stats() == stats
    assert held.report(S).tobytes() == before
    with pytest.raises(Exception):
        held.report(S, keep=[n])
    # no held state: a score pass replaces it
    ss.score(S, 11, 2, rectangle(0, 2, 0, 2))
    assert report() == INV and filt() == INV
    assert rep.tobytes() == bytes([7]) * 80 and pos.tolist() == [7, 7] and count.value == 77


def rows_of(capsys, argv):
    assert allpairs.main(argv) == 0
    return capsys.readouterr().out.splitlines()


def test_the_command(capsys):
    path = os.path.join(ROOT, "tests", "golden", "protein.fasta")
    records = read_fasta(path)
    heads = [r.head.decode("utf-8", "replace") for r in records]
    codes = encode_records(records, Protein)
    S = get_blosum62()

    def columns(held, h, r):
        x = report_fractions(np.array([r]), [len(codes[int(held.q[h])])], [len(codes[int(held.t[h])])])[0]
        return ",%d,%r,%r,%r,%r,%d,%d" % (int(r["columns"]), float(x["identity"]), float(x["positives"]), float(x["q_cover"]), float(x["t_cover"]),
                                          int(r["q_gap_open"]) + int(r["t_gap_open"]), int(r["q_gap"]) + int(r["t_gap"]))

    with SeqSet(codes) as ss:
        # --best 3: what the command prints without the new flags, from SeqSet calls
        held = ss.best(S, 11.0, 2.0, 3, skip_self=True)
        plain = ["%s,%d,%s,%r" % (heads[q], int(held.rank[p]) + 1, heads[int(held.t[p])], float(held.f[p])) for q, pos in held.by_query() for p in pos]
        order = [int(p) for q, pos in held.by_query() for p in pos]
        ref = oracle_strings(codes, oracle.CORE_LOCAL, held.q, held.t, S)
        model = report_ref.reports(ref, S, SKIP)
        want_best = [row + columns(held, h, model[h]) for row, h in zip(plain, order)]
        # --f-min F
        f_min = 30.0
        hits = ss.hits(S, 11.0, 2.0, f_min, None)
        assert len(hits) > 0
        plain_hits = ["%s,%s,%r" % (heads[int(q)], heads[int(t)], float(f)) for q, t, f in zip(hits.q, hits.t, hits.f)]
        ref = oracle_strings(codes, oracle.CORE_LOCAL, hits.q, hits.t, S)
        model_hits = report_ref.reports(ref, S, SKIP)
        lens = np.array([len(c) for c in codes])
        kept = np.flatnonzero(report_ref.keep(model_hits, lens[hits.q], lens[hits.t], min_identity=0.5))
        low = np.flatnonzero(report_ref.keep(model_hits, lens[hits.q], lens[hits.t], min_identity=0.05, min_q_cover=0.1, min_t_cover=0.1))
        some = np.flatnonzero(report_ref.keep(model_hits, lens[hits.q], lens[hits.t], min_identity=0.05))
        assert len(low) > 0 and len(some) > 0
    assert rows_of(capsys, ["-i", path, "--best", "3"]) == plain and len(plain) > 0
    assert rows_of(capsys, ["-i", path, "--best", "3", "--report"]) == want_best
    assert rows_of(capsys, ["-i", path, "--f-min", "30"]) == plain_hits
    assert rows_of(capsys, ["-i", path, "--f-min", "30", "--min-identity", "0.5", "--report"]) == \
        [plain_hits[h] + columns(hits, h, model_hits[h]) for h in kept]
    assert rows_of(capsys, ["-i", path, "--f-min", "30", "--min-identity", "0.05", "--min-q-cover", "0.1", "--min-t-cover", "0.1"]) == \
        [plain_hits[h] for h in low]
    # with --shuffles the new columns come after z,p_emp, and the copies are drawn for the kept hits
    more = rows_of(capsys, ["-i", path, "--f-min", "30", "--shuffles", "50", "--report", "--min-identity", "0.05"])
    sig = rows_of(capsys, ["-i", path, "--f-min", "30", "--shuffles", "50"])
    assert more == [sig[h] + columns(hits, h, model_hits[h]) for h in some]
