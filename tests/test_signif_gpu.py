"""Significance of a sequence set's held hits (aln_seqset_held_significance, HeldHits.significance / p_values): the per-copy scores
bit for bit against aln_shuffle_scores on the same pair and stream and against the oracle on restated copies, the records against
the numpy restatement of the rule (signif_ref.py) for integer, all-zero, negative and real-valued scores, failed copies, independence
of the held pass, of keep and of the chunking, the held state before and after, the p-values against the host fit, the refusals."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shuffle_ref  # noqa: E402
import signif_ref  # noqa: E402
from aligner_amd import _ffi, allpairs, runtime, statistics  # noqa: E402
from aligner_amd.batch import PairBatch, align_batch  # noqa: E402
from aligner_amd.matrices import get_blosum62  # noqa: E402
from aligner_amd.seqset import SIGNIF_RECORD_DTYPE, SeqSet, rectangle, significance_from_records  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED51
BASE = 1000                        # pair_base of the calls below: stream = BASE + the hit's pair number
F_MIN = 20.0
LENGTHS = [5, 6, 7, 63, 64, 65, 130, 513, 600, 2100]
BAD = 10                           # the sequence with a code outside the matrix


def the_sequences():
    """11 proteins from a fixed seed.  A 40-residue motif whose first seven residues are the four with the highest self-score lies in
    every one of them (the three shortest ARE its first 5, 6, 7 residues), so hits exist at every length; sequence 10 also holds
    code 30."""
    S = get_blosum62()
    rng = np.random.default_rng(20261018)
    top = np.argsort(-np.diag(S)[:20], kind="stable")[:4]
    motif = rng.integers(0, 20, 40).astype(np.uint8)
    motif[:7] = top[[0, 1, 0, 2, 0, 3, 1]]
    seqs = []
    for L in LENGTHS:
        if L < 40:
            seqs.append(motif[:L].copy())
            continue
        s = rng.integers(0, 20, L).astype(np.uint8)
        at = int(rng.integers(0, L - 40 + 1))
        s[at:at + 40] = motif
        seqs.append(s)
    bad = rng.integers(0, 20, 80).astype(np.uint8)
    bad[10:50] = motif
    bad[60] = 30
    seqs.append(bad)
    return seqs


def schemes():
    S = get_blosum62()
    return {"local_11_2": (_ffi.CORE_LOCAL, 11, 2, S),
            "core_global_4_4": (_ffi.CORE_GLOBAL, 4, 4, S),                 # Alignment.f of the core global aligner is 0.0
            "legacy_global_4": (_ffi.LEGACY_GLOBAL, 4, 4, S),               # f = H[M][N]: negative for shuffled copies
            "real_f64": (_ffi.CORE_LOCAL, 10.7, 1.3, S * 1.1 + 0.013)}      # not a multiple of 2^-k for any k <= 8: the f64 kernels


def raw(held, scheme, per_pair, keep, scores=True, seed=SEED, pair_base=BASE, max_trim=6, fill=None, records="own"):
    """aln_seqset_held_significance through ctypes: (status of the call, records, f, lengths); the outputs start as `fill` bytes."""
    sem, d, e, S = scheme
    o = held.owner
    keep = np.ascontiguousarray(keep, dtype=np.uint32)
    n = len(keep)
    p, _alive = runtime.make_params(sem, d, e, S, outputs=_ffi.OUT_SCORE)
    spec = _ffi.ShuffleSpec(seed, pair_base, per_pair, max_trim)
    rec = np.full(48 * max(n, 1), 0 if fill is None else fill, dtype=np.uint8).view(SIGNIF_RECORD_DTYPE)[:n]
    m = n * min(max(per_pair, 1), 1 << 20) if scores else 0
    f = np.full(8 * max(m, 1), 0 if fill is None else fill, dtype=np.uint8).view(np.float64)[:m]
    L = np.full(4 * max(m, 1), 0 if fill is None else fill, dtype=np.uint8).view(np.uint32)[:m]
    st = o.lib.aln_seqset_held_significance(o.handle, C.byref(p), C.byref(spec), keep.ctypes.data, n, rec.ctypes.data if records == "own" else records,
                                            f.ctypes.data if scores else None, L.ctypes.data if scores else None)
    if scores and st == 0:
        f, L = f.reshape(n, per_pair), L.reshape(n, per_pair)
    return st, rec, f, L


def copy_status(sem, f, L):
    """Per-copy status out of the scores and lengths of aln_shuffle_scores (the baseline, never the call under test): a copy trimmed to
    nothing is the reference's empty-sequence panic; a local alignment without a positive cell has f = 0 (every other local f is
    positive).  base_status checks the first of them against the status aln_shuffle_scores itself reports for the pair."""
    st = np.zeros(f.shape, dtype=np.int32)
    if sem in (_ffi.CORE_LOCAL, _ffi.LEGACY_LOCAL):
        st[f == 0.0] = _ffi.ERR_NO_POSITIVE_CELL
    st[L == 0] = _ffi.ERR_EMPTY_SEQUENCE
    return st


@pytest.fixture(scope="module")
def seqs():
    return the_sequences()


@pytest.fixture(scope="module")
def ss(seqs):
    with SeqSet(seqs) as s:
        yield s


def hold(ss):
    n = len(ss)
    return ss.hits(get_blosum62(), 11, 2, F_MIN, rectangle(0, n, 0, n))


@pytest.fixture()
def held(ss):
    """(held again for every test: some tests end with another pass on the set)"""
    h = hold(ss)
    # hits at every length, none with the sequence that cannot be aligned
    assert set(range(10)) <= set(h.t.tolist()) and set(range(10)) <= set(h.q.tolist())
    assert BAD not in h.q.tolist() and BAD not in h.t.tolist()
    return h


def listable(held, max_target=None):
    """positions whose target is not the 5-residue one (shorter than max_trim = 6)"""
    tl = held.owner.len[held.t]
    ok = tl >= 6
    if max_target is not None:
        ok &= tl <= max_target
    return np.flatnonzero(ok).astype(np.uint32)


@pytest.fixture(scope="module")
def baseline(ss, seqs):
    """aln_shuffle_scores on one pair under the stream of its pair number (tested on its own in test_shuffle_gpu.py), computed once
    per (pair, scheme, per_pair)"""
    memo = {}

    def get(q, t, index, name, per_pair):
        key = (q, t, name, per_pair)
        if key not in memo:
            sem, d, e, S = schemes()[name]
            f, L, st = statistics.device_shuffled_scores([(seqs[q], seqs[t])], d, e, S, SEED, per_pair=per_pair, max_trim=6, pair_base=BASE + index,
                                                         semantics=sem, check=False)
            memo[key] = (f[0], L[0], int(st[0]))
        return memo[key]
    return get


def base_status(held, baseline, name, per_pair, keep):
    """(f, lengths, per-copy status) of the listed hits from the baseline alone"""
    sem = schemes()[name][0]
    f, L = np.zeros((len(keep), per_pair)), np.zeros((len(keep), per_pair), dtype=np.uint32)
    for k, h in enumerate(keep):
        f[k], L[k], bst = baseline(int(held.q[h]), int(held.t[h]), int(held.index[h]), name, per_pair)
        bad = np.flatnonzero(copy_status(sem, f[k], L[k]))
        assert bst == (int(copy_status(sem, f[k], L[k])[bad[0]]) if len(bad) else 0), (k, h)
    return f, L, copy_status(sem, f, L)


# ---------------------------------------------------------------- the per-copy scores
def test_copies_are_those_of_shuffle_scores_under_the_pair_number(held, baseline):
    """keep in descending order with duplicates: a stream indexed by the position in keep or in the held list would differ."""
    w = listable(held)
    keep = np.concatenate([w[::-1], w[:2], w[-1:]])
    st, rec, f, L = raw(held, schemes()["local_11_2"], 64, keep)
    assert st == 0
    assert not (held.index[w] == np.arange(len(w))).all()             # the pair number is not the position
    for k, h in enumerate(keep):
        bf, bL, bst = baseline(int(held.q[h]), int(held.t[h]), int(held.index[h]), "local_11_2", 64)
        assert f[k].tobytes() == bf.tobytes() and (L[k] == bL).all(), (k, h)
        assert int(rec["status"][k]) == bst
    assert rec[len(w)].tobytes() == rec[len(w) - 1].tobytes() and f[len(w)].tobytes() == f[len(w) - 1].tobytes()


def test_copies_equal_the_oracle_on_restated_copies(held, seqs, orc):
    """One target shuffled in LDS (130 residues) and the 2 100-residue one (in place in global memory), 64 copies each."""
    S = get_blosum62()
    pick = [int(np.flatnonzero((held.q == 3) & (held.t == t))[0]) for t in (6, 9)]
    st, rec, f, L = raw(held, schemes()["local_11_2"], 64, pick)
    assert st == 0
    for k, h in enumerate(pick):
        q, t = seqs[int(held.q[h])], seqs[int(held.t[h])]
        copies = [shuffle_ref.copy_of(t, SEED, BASE + int(held.index[h]), s, 6)[1] for s in range(64)]
        assert L[k].tolist() == [len(c) for c in copies]
        b = PairBatch.from_pairs([(q, c) for c in copies])
        ref, _, _ = orc.align_batch(_ffi.CORE_LOCAL, b.seqs, b.q_off, b.q_len, b.t_off, b.t_len, 11, 2, S, n_threads=16, want_traceback=False)
        assert f[k].tolist() == [r.f for r in ref]
        assert rec["n_ok"][k] == 64 and rec["status"][k] == 0


# ---------------------------------------------------------------- the records
def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("per_pair", [1, 63, 64, 65, 130, 4999])
@pytest.mark.parametrize("name", ["local_11_2", "core_global_4_4", "legacy_global_4", "real_f64"])
def test_records_follow_the_rule(held, baseline, name, per_pair):
    """The reference of every record is the rule's restatement applied to what aln_shuffle_scores gives for the pair on its own."""
    scheme = schemes()[name]
    keep = listable(held, 130 if per_pair == 4999 else None)
    st, rec, f, L = raw(held, scheme, per_pair, keep)
    assert st == 0 and len(keep) > 20
    bf, bL, status = base_status(held, baseline, name, per_pair, keep)
    assert f.tobytes() == bf.tobytes() and (L == bL).all()
    want = signif_ref.reduce_many(bf, status, held.f[keep])
    for k in range(len(keep)):
        assert rec[k].tobytes() == want[k].tobytes(), (k, rec[k], want[k])
    # without the scores: the same records
    st2, rec2, _, _ = raw(held, scheme, per_pair, keep, scores=False)
    assert st2 == 0 and rec2.tobytes() == rec.tobytes()
    ok = status == 0
    if name == "core_global_4_4":
        assert (f[ok] == 0.0).all()                                   # (simple/mod.rs:139: the global aligner's f)
    if name == "legacy_global_4" and per_pair >= 63:
        # every score of some hit is negative: a maximum that started at 0, or an unsigned compare, would show
        assert ((rec["f_max"] < 0) & (rec["n_ok"] > 0)).any() and (rec["n_ge"][rec["f_max"] < 0] == 0).all()
    if name == "real_f64" and per_pair >= 63:
        # the order is under test only if it shows: for some listed hit one ascending sum gives other bits than the rule
        seq = [signif_ref.sequential(f[k], status[k]) for k in range(len(keep))]
        assert any(bits(rec["sum"][k]) != bits(s[0]) or bits(rec["sum_sq"][k]) != bits(s[1]) for k, s in enumerate(seq))
        assert (f[ok] != np.round(f[ok] * 256) / 256).any()           # not dyadic: the f64 kernels' own numbers


def test_failed_copies_are_counted_by_their_absence(held, baseline):
    """The 6-residue target under max_trim = 6: a seventh of its copies is trimmed to nothing.  The hits on other targets in the same
    call are what they are without it.  Listing a hit on the 5-residue target refuses the whole call."""
    scheme = schemes()["local_11_2"]
    keep = listable(held)
    six = np.flatnonzero(held.t[keep] == 1)
    assert len(six) >= 3
    st, rec, f, L = raw(held, scheme, 64, keep)
    assert st == 0
    bf, bL, status = base_status(held, baseline, "local_11_2", 64, keep)
    assert f.tobytes() == bf.tobytes() and (L == bL).all()
    for k in six:
        empty = np.flatnonzero(shuffle_ref.trims(SEED, BASE + int(held.index[keep[k]]), 64, 6) == 6)
        assert len(empty) > 0 and (L[k][empty] == 0).all() and rec["n_ok"][k] <= 64 - len(empty)
        bad = np.flatnonzero(status[k])
        assert rec["first_bad"][k] == bad[0] and rec["n_ok"][k] == 64 - len(bad)
        assert rec["status"][k] == (_ffi.ERR_EMPTY_SEQUENCE if L[k][bad[0]] == 0 else _ffi.ERR_NO_POSITIVE_CELL)
    assert (rec["status"][six] != 0).all()
    rest = np.delete(np.arange(len(keep)), six)
    st, rec_rest, f_rest, _ = raw(held, scheme, 64, keep[rest])
    assert st == 0 and rec_rest.tobytes() == rec[rest].tobytes() and f_rest.tobytes() == f[rest].tobytes()
    five = int(np.flatnonzero(held.t == 0)[0])
    st, rec5, f5, L5 = raw(held, scheme, 64, np.concatenate([keep[:3], [five]]), fill=0xA5)
    assert st == _ffi.ERR_INVALID_ARGUMENT
    assert (rec5.view(np.uint8) == 0xA5).all() and (f5.view(np.uint8) == 0xA5).all() and (L5.view(np.uint8) == 0xA5).all()
    assert raw(held, scheme, 64, np.concatenate([keep[:3], [five]]), max_trim=5)[0] == 0


# ---------------------------------------------------------------- independence
def test_a_pairs_record_does_not_depend_on_the_held_pass_or_on_keep(ss, held):
    scheme = schemes()["real_f64"]
    n = len(ss)
    keep = listable(held)
    st, rec, f, _ = raw(held, scheme, 130, keep)
    assert st == 0
    # alone, and between other entries
    for k in (0, len(keep) // 2, len(keep) - 1):
        st, one, f1, _ = raw(held, scheme, 130, keep[k:k + 1])
        assert st == 0 and one[0].tobytes() == rec[k].tobytes() and f1[0].tobytes() == f[k].tobytes()
    by_pair = {int(held.index[h]): k for k, h in enumerate(keep)}
    held_f = {int(held.index[h]): float(held.f[h]) for h in keep}
    # the k best of the same block: other positions, the same pair numbers
    best = ss.best(get_blosum62(), 11, 2, 3, block=rectangle(0, n, 0, n))
    bkeep = listable(best)
    common = [int(h) for h in bkeep if int(best.index[h]) in by_pair]
    assert len(common) >= 10 and any(int(h) != int(keep[by_pair[int(best.index[h])]]) for h in common)
    st, brec, bf, _ = raw(best, scheme, 130, common)
    assert st == 0
    for k, h in enumerate(common):
        pair = int(best.index[h])
        assert float(best.f[h]) == held_f[pair]
        assert brec[k].tobytes() == rec[by_pair[pair]].tobytes() and bf[k].tobytes() == f[by_pair[pair]].tobytes()


def digest(rec, f):
    return hashlib.sha256(rec.tobytes() + f.tobytes()).hexdigest()


CHILD = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_signif_gpu as T
from aligner_amd.seqset import SeqSet
with SeqSet(T.the_sequences()) as ss:
    held = T.hold(ss)
    st, rec, f, L = T.raw(held, T.schemes()["real_f64"], 64, T.listable(held))
    assert st == 0
    print("DIGEST", T.digest(rec, f))
"""


def test_small_chunks_give_the_same_bytes(held):
    """ALN_CHUNK_CELLS = 3e6 in a child process: the job is cut into many chunks of whole hits (the count is the library's own, from
    its plan trace), records and scores hash as the unchunked ones."""
    st, rec, f, _ = raw(held, schemes()["real_f64"], 64, listable(held))
    assert st == 0
    env = dict(os.environ, ALN_CHUNK_CELLS="3e6", ALN_TRACE_PLAN="1")
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.dirname(os.path.abspath(__file__)))], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    chunks = [int(m.group(1)) for m in re.finditer(r"aln shuffle: pairs \d+ copies 64 chunks (\d+)", out.stderr)]
    assert chunks and chunks[-1] >= 4, out.stderr[-2000:]
    assert re.search(r"DIGEST (\w+)", out.stdout).group(1) == digest(rec, f)


# ---------------------------------------------------------------- held state
def test_held_state_survives_and_other_calls_do_not_disturb(ss, held, seqs):
    scheme = schemes()["local_11_2"]
    S = get_blosum62()
    keep = listable(held)
    res0, str0 = held.strings()
    st, rec, f, _ = raw(held, scheme, 65, keep)
    assert st == 0
    res1, str1 = held.strings()
    assert res0.tobytes() == res1.tobytes()
    assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(str0, str1))
    again = hold(ss)                                                   # (the list itself, from the host)
    assert (again.index == held.index).all() and again.f.tobytes() == held.f.tobytes()
    # other calls on the same context in between
    align_batch(PairBatch.from_pairs([(seqs[7], seqs[8]), (seqs[3], seqs[9])]), _ffi.CORE_LOCAL, 11, 2, S)
    statistics.device_shuffled_scores([(seqs[6], seqs[7])], 11, 2, S, seed=3, per_pair=200)
    st, rec2, f2, _ = raw(again, scheme, 65, keep)
    assert st == 0 and rec2.tobytes() == rec.tobytes() and f2.tobytes() == f.tobytes()
    stats = ss.stats()
    assert stats["bytes_down"] == 48 * len(keep) + 8 * 65 * len(keep) and stats["fetch_kernel_ms"] > 0
    st, _, _, _ = raw(again, scheme, 65, keep, scores=False)
    assert st == 0 and ss.stats()["bytes_down"] == 48 * len(keep)
    # a score pass replaces the held state: refused, nothing written
    ss.score(S, 11, 2, rectangle(0, 3, 3, 2))
    st, rec3, f3, _ = raw(again, scheme, 65, keep, fill=0xA5)
    assert st == _ffi.ERR_INVALID_ARGUMENT and (rec3.view(np.uint8) == 0xA5).all() and (f3.view(np.uint8) == 0xA5).all()


# ---------------------------------------------------------------- on top: z, p_emp, p-values
def test_significance_and_p_values(held, baseline, seqs):
    S = get_blosum62()
    pick = [int(np.flatnonzero((held.q == q) & (held.t == t))[0]) for q, t in ((3, 6), (6, 4), (5, 3))]
    sig, f, L = held.significance(S, 11, 2, SEED, keep=pick, pair_base=BASE, scores=True)
    got = held.p_values(S, 11, 2, SEED, keep=pick, pair_base=BASE, slice_hits=2)
    for k, h in enumerate(pick):
        q, t = int(held.q[h]), int(held.t[h])
        bf, bL, bst = baseline(q, t, int(held.index[h]), "local_11_2", 4999)
        assert bst == 0 and f[k].tobytes() == bf.tobytes()
        fh = float(held.f[h])
        scores = np.concatenate([[fh], bf])
        lengths = np.concatenate([[len(seqs[t])], bL.astype(np.int64)])
        want = statistics.calculate_distribution_params(len(seqs[q]), lengths, scores).get_p_value(len(seqs[q]), len(seqs[t]), fh)
        np.testing.assert_array_equal(got[k], want)
        rec = signif_ref.reduce_one(bf, np.zeros(4999, dtype=np.int32), fh)
        mine = significance_from_records(rec.reshape(1), [fh])[0]
        assert sig[k].tobytes() == mine.tobytes()
        assert sig["p_emp"][k] == (int((bf >= fh).sum()) + 1) / 5000.0 and abs(sig["mean"][k] - bf.mean()) < 1e-9
    assert (sig["z"] > 5).all() and (sig["p_emp"] < 0.01).all()       # the shared 40-residue motif is not a chance hit


# ---------------------------------------------------------------- refusals
def test_refusals_write_nothing(held):
    local = schemes()["local_11_2"]
    keep = listable(held)[:4]
    pwm = (_ffi.PWM_LOCAL, 5, 5, np.random.default_rng(1).integers(-2, 3, (4, 30)).astype(np.float64))
    cases = [(pwm, 10, keep, _ffi.ERR_UNSUPPORTED),
             (local, 0, keep, _ffi.ERR_INVALID_ARGUMENT),
             (local, (1 << 20) + 1, keep, _ffi.ERR_INVALID_ARGUMENT),
             (local, 10, np.array([0, len(held)], dtype=np.uint32), _ffi.ERR_INVALID_ARGUMENT)]
    for scheme, per_pair, w, want in cases:
        st, rec, f, L = raw(held, scheme, per_pair, w, fill=0xA5)
        assert st == want, (per_pair, st)
        assert (rec.view(np.uint8) == 0xA5).all() and (f.view(np.uint8) == 0xA5).all() and (L.view(np.uint8) == 0xA5).all()
    st, _, f, L = raw(held, local, 10, keep, fill=0xA5, records=None)
    assert st == _ffi.ERR_INVALID_ARGUMENT and (f.view(np.uint8) == 0xA5).all() and (L.view(np.uint8) == 0xA5).all()
    assert raw(held, local, 10, keep[:0])[0] == 0                      # nothing listed is nothing to do
    res, _ = held.strings(keep)                                        # the held state is intact
    assert (res["status"] == 0).all() and res["f"].tolist() == held.f[keep].tolist()


# ---------------------------------------------------------------- hits that lie far apart in the set's buffer
def test_hits_far_apart_are_copied_range_by_range(seqs):
    """A 200 000-residue sequence between the two of the only hit: the listed residues are gathered on the device range by range
    instead of as one span.  The same bytes as the pair on its own."""
    S = get_blosum62()
    filler = np.random.default_rng(4).integers(0, 20, 200000).astype(np.uint8)
    with SeqSet([seqs[6], filler, seqs[7]]) as far:
        held = far.hits(S, 11, 2, F_MIN, rectangle(0, 1, 2, 1))
        assert len(held) == 1
        st, rec, f, L = raw(held, schemes()["local_11_2"], 130, [0])
        assert st == 0
        bf, bL, bst = statistics.device_shuffled_scores([(seqs[6], seqs[7])], 11, 2, S, SEED, per_pair=130, pair_base=BASE + int(held.index[0]))
        assert f[0].tobytes() == bf[0].tobytes() and (L[0] == bL[0]).all()
        assert rec[0].tobytes() == signif_ref.reduce_one(bf[0], np.zeros(130, dtype=np.int32), held.f[0]).tobytes()


# ---------------------------------------------------------------- the command
def test_allpairs_appends_z_and_p(tmp_path, seqs, capsys):
    from aligner_amd.enums import Protein
    path = str(tmp_path / "x.fasta")
    with open(path, "w") as fh:
        for i in (3, 4, 5, 6, 2, 0):                                   # s0 has 5 residues: no copies of it as a target
            fh.write(">s%d\n%s\n" % (i, Protein.vec_to_str(seqs[i])))
    for held_args in (["--best", "5"], ["--f-min", "30"]):               # (five partners: every other record, s0 among them)
        assert allpairs.main(["-i", path] + held_args) == 0
        plain = capsys.readouterr().out.splitlines()
        assert allpairs.main(["-i", path] + held_args + ["--shuffles", "200", "--seed", "7"]) == 0
        more = capsys.readouterr().out.splitlines()
        assert len(plain) == len(more) > 0
        short = 0
        for a, b in zip(plain, more):
            assert b.startswith(a + ",") and len(b[len(a) + 1:].split(",")) == 2
            if a.split(",")[-2] == "s0":                               # (the target's head stands in front of f)
                assert b[len(a):] == ",nan,nan"
                short += 1
                continue
            z, p = [float(v) for v in b[len(a) + 1:].split(",")]
            assert 0 < p <= 1 and z == z
        assert short > 0
