"""CIGARs on the device (aln_seqset_held_cigar_plan / _fill, HeldHits.cigars) against the plain Python rule of cigar_ref.py fed from
held.strings() and the summaries of the same held pass: every record, offset, word and summary field for equality, and decode of the
device's words over the set's own residues against held.strings() without the seed column.  The hand-built set's properties -- gap
runs that end on both sides of the round edges, a gap run longer than a round, hits of exactly 63, 64 and 65 columns -- are asserted
from the strings before anything is compared."""
import ctypes as C
import hashlib
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cigar_ref as R  # noqa: E402
import cluster_cases  # noqa: E402
from aligner_amd import _ffi, allpairs, cigar  # noqa: E402
from aligner_amd import build as native_build  # noqa: E402
from aligner_amd.enums import Protein  # noqa: E402
from aligner_amd.fasta import encode_records, read_fasta  # noqa: E402
from aligner_amd.matrices import get_blosum62  # noqa: E402
from aligner_amd.seqset import SeqSet, rectangle  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLANK = 98
DEL, EXT = 4.0, 1.0           # low gap costs for the hand-built set: its inserts are bridged, not cut
ALL_FLAGS = (0, R.EXTENDED, R.CLIPS, R.EXTENDED | R.CLIPS)
ENDS = (62, 63, 64, 65, 126, 127, 128, 129)


def hand_built():
    """32 records of at most 330 residues: a centre of 200, a part of it between unrelated flanks (a query with clips), copies with an
    insert or a deletion whose gap run ends at the columns of ENDS, two with inserts of 60 to 70, and four prefixes of an unrelated
    sequence that align in exactly 63, 64 and 65 columns."""
    rng = np.random.default_rng(2020)
    w = int(Protein.str_to_vec("W")[0])               # the long inserts are all W and the centre has none: no column of them pairs up
    centre = rng.integers(0, 19, size=200).astype(np.uint8)
    centre[centre >= w] += 1
    recs = [centre, np.concatenate([rng.integers(0, 20, size=6), centre[10:190], rng.integers(0, 20, size=9)]).astype(np.uint8)]
    for e in ENDS:
        for width in (2, 5):
            recs.append(np.insert(centre, e - width + 1, rng.integers(0, 20, size=width).astype(np.uint8)))
        recs.append(np.delete(centre, np.arange(e - 3, e + 1)))
    recs.append(np.insert(centre, 30, np.full(70, w, dtype=np.uint8)))
    recs.append(np.insert(np.insert(centre, 150, np.full(60, w, dtype=np.uint8)), 20, np.full(66, w, dtype=np.uint8)))
    other = rng.integers(0, 20, size=66).astype(np.uint8)
    recs += [other[:63].copy(), other[:64].copy(), other[:65].copy(), other[:66].copy()]
    assert len(recs) == 32 and max(len(r) for r in recs) <= 330
    return recs


def gap_runs(qs, ts, n):
    """[(first column, length)] of the maximal runs of columns with a blank on one side"""
    runs, j = [], 0
    while j < n:
        side = 1 if qs[j] == BLANK else 2 if ts[j] == BLANK else 0
        k = j + 1
        while k < n and (1 if qs[k] == BLANK else 2 if ts[k] == BLANK else 0) == side:
            k += 1
        if side:
            runs.append((j, k - j))
        j = k
    return runs


class Case:
    """a held pass and its reference entries, computed once and left unchanged"""

    def __init__(self, held):
        self.held = held
        self.entries, (self.res, self.strs, self.seqs) = R.entries_of(held, BLANK)
        self.whole = {}                                   # flags -> the reference of the whole list

    def check(self, which=None, flags=0):
        held = self.held
        w = list(range(len(held))) if which is None else [int(h) for h in which]
        got = held.cigars(keep=None if which is None else np.array(w, dtype=np.uint32), extended=bool(flags & R.EXTENDED), clips=bool(flags & R.CLIPS))
        fill_stats = held.owner.stats()
        if which is not None:
            recs, off, words, summ = R.listed(self.entries, w, len(held), BLANK, flags)
        else:
            if flags not in self.whole:
                self.whole[flags] = R.listed(self.entries, w, len(held), BLANK, flags)
            recs, off, words, summ = self.whole[flags]
        assert got.summary == summ and summ["overflow"] == 0 and summ["padded"] == 0 and summ["failed"] == 0
        assert got.records.dtype == cigar.CIGAR_RECORD_DTYPE and [tuple(int(x) for x in r) for r in got.records.tolist()] == recs
        assert got.offsets.dtype == np.uint64 and got.offsets.tolist() == off
        assert got.words.dtype == np.uint32 and got.words.tolist() == words
        assert len(got) == len(w) and got.which.tolist() == w
        for i, h in enumerate(w):                         # the round trip over the set's own residues
            r = got.records[i]
            n = R.counted_columns(int(self.res["aln_len"][h]))
            qs, ts = cigar.decode(got.ops(i), self.seqs[int(held.q[h])], self.seqs[int(held.t[h])], int(r["q_start"]), int(r["t_start"]), BLANK)
            assert qs.tolist() == self.strs[h][0][:n].tolist() and ts.tolist() == self.strs[h][1][:n].tolist(), h
            assert got.text(i) == R.text(words[off[i]:off[i + 1]])
        plan = held.last_cigar_plan_stats
        assert plan["bytes_up"] == 4 * len(w) and plan["bytes_down"] == 32 * len(w) + 32
        assert fill_stats["bytes_up"] == 0 and fill_stats["bytes_down"] == 4 * summ["total_ops"] + 8 * (len(w) + 1)
        return got


@pytest.fixture(scope="module")
def local():
    S = get_blosum62()
    with SeqSet(hand_built()) as ss:
        yield ss, S, Case(ss.hits(S, DEL, EXT, 150.0, None))


def test_the_hand_built_set_has_what_it_is_built_for(local):
    ss, S, case = local
    held, res, strs = case.held, case.res, case.strs
    assert len(held) > 256, "more than one tile of the offset scan"
    n_of = [R.counted_columns(int(a)) for a in res["aln_len"]]
    runs = [r for h in range(len(held)) for r in gap_runs(strs[h][0], strs[h][1], n_of[h])]
    for e in ENDS:
        assert any(a + n - 1 == e for a, n in runs), "a gap run ends at column %d" % e
    assert any(n > 64 for a, n in runs), "a gap run longer than a round"
    assert any(a < 64 and a + n > 128 for a, n in runs) or any(n >= 66 for a, n in runs)
    for n in (63, 64, 65):
        assert n in n_of, "a hit of exactly %d counted columns" % n
    assert any(not gap_runs(strs[h][0], strs[h][1], n_of[h]) for h in range(len(held))), "a hit without any gap"
    got = case.check()
    gapless = [i for i in range(len(held)) if not gap_runs(strs[i][0], strs[i][1], n_of[i])]
    assert all(got.ops(i).tolist() == [(n_of[i] << 4) | R.M] for i in gapless), "a hit without any gap: one M word"
    assert max(int(w) >> 4 for w in got.words if int(w) & 15 in (R.I, R.D)) >= 66


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_every_flag_combination(local, flags):
    ss, S, case = local
    got = case.check(flags=flags)
    ops = set(int(w) & 15 for w in got.words)
    assert (R.EQ in ops and R.X in ops and R.M not in ops) if flags & R.EXTENDED else (R.M in ops and R.EQ not in ops and R.X not in ops)
    lens = ss.len[case.held.q]
    clipped = (got.records["q_start"] > 0) | (got.records["q_end"] < lens)
    assert clipped.any() and ((R.S in ops) == bool(flags & R.CLIPS))
    if flags & R.CLIPS:
        for i in np.flatnonzero(clipped)[:20].tolist():
            w = got.ops(i).tolist()
            r = got.records[i]
            lead, trail = int(r["q_start"]), int(lens[i]) - int(r["q_end"])
            assert (w[0] == (lead << 4) | R.S) == (lead > 0) and (w[-1] == (trail << 4) | R.S) == (trail > 0)
            assert sum(x >> 4 for x in w if x & 15 in (R.M, R.I, R.S, R.EQ, R.X)) == int(lens[i]), "with clips the words consume the whole query"


def test_lists(local):
    ss, S, case = local
    n = len(case.held)
    full = case.check()
    sub = case.check(which=list(range(3, n, 7)))
    assert sub.ops(1).tolist() == full.ops(10).tolist()
    down = case.check(which=list(range(n - 1, -1, -1)), flags=R.EXTENDED)
    assert int(down.offsets[-1]) == down.summary["total_ops"]
    twice = case.check(which=[5, 5, 300, 5, 0, 300])
    assert twice.ops(0).tolist() == twice.ops(1).tolist() == twice.ops(3).tolist() == full.ops(5).tolist()
    none = case.check(which=[])
    assert len(none) == 0 and none.offsets.tolist() == [0] and len(none.words) == 0 and none.summary["held"] == n
    one = case.check(which=[n - 1], flags=R.CLIPS)
    assert len(one) == 1


def test_global_and_real_valued_schemes():
    rng = np.random.default_rng(5)
    centre = rng.integers(0, 20, size=70).astype(np.uint8)
    recs = [centre, np.concatenate([rng.integers(0, 20, size=5), centre, rng.integers(0, 20, size=4)]).astype(np.uint8),
            np.concatenate([rng.integers(0, 20, size=2), centre[:30], centre[33:], rng.integers(0, 20, size=7)]).astype(np.uint8), centre[3:60].copy()]
    S = get_blosum62()
    with SeqSet(recs) as ss:
        case = Case(ss.hits(S, 4.0, 4.0, 0.0, rectangle(0, 4, 0, 4), semantics=_ffi.CORE_GLOBAL))
        assert len(case.held) == 16
        firsts = [gap_runs(s[0], s[1], len(s[0]) - 1)[:1] for s in case.strs]
        assert any(f and f[0][0] == 0 for f in firsts), "a hit begins with a gap"
        for flags in ALL_FLAGS:
            got = case.check(flags=flags)
            assert (got.records["q_start"] == 0).all() and (got.records["q_end"] == ss.len[case.held.q]).all() and R.S not in set(int(w) & 15 for w in got.words)
        real = S * 0.37 + 0.011                           # no multiple of a power of two: the real-valued kernels
        case = Case(ss.hits(real, 3.3, 1.1, 5.0, None))
        assert len(case.held) >= 3 and not (case.res["flags"] & 1).any(), "the real-valued route"
        for flags in (0, R.EXTENDED | R.CLIPS):
            case.check(flags=flags)


def test_after_every_kind_of_held_pass(local):
    ss, S, _case = local
    n = len(ss)
    try:
        Case(ss.best(S, DEL, EXT, 3, skip_self=True)).check(flags=R.EXTENDED)
        cand = ss.prefilter(3, 20, min_shared=0, min_per_1024=128, block=rectangle(0, n, 0, n))
        assert 0 < len(cand) < n * n
        Case(cand.hits(S, DEL, EXT, 150.0)).check(flags=R.CLIPS)
        Case(cand.best(S, DEL, EXT, 4, skip_self=True)).check(flags=R.EXTENDED | R.CLIPS)
    finally:
        _case.held = ss.hits(S, DEL, EXT, 150.0, None)    # (the fixture's pass again: the same hits, the same strings)


# ---------------------------------------------------------------- plans and fills, the held state, the refusals
def digest(held, S, labels):
    lst = held.__class__(held.owner, len(held), held.semantics)       # (held_list again)
    res, strs = held.strings()
    clusters = held.cluster(S, mode="greedy", min_identity=0.3)
    h = hashlib.sha256()
    for part in (lst.index, lst.q, lst.t, lst.f, res, held.report(S), held.filter(S, min_identity=0.5), clusters.label, held.profiles(labels).out,
                 held.msa(labels).out):
        h.update(np.ascontiguousarray(part).tobytes())
    for x, y in strs:
        h.update(x.tobytes())
        h.update(y.tobytes())
    return h.hexdigest()


def test_state_plans_and_refusals(local):
    ss, S, case = local
    lib, held = ss.lib, case.held
    n = len(held)
    labels = np.zeros(len(ss), dtype=np.uint32)
    before = digest(held, S, labels)
    s0 = ss.stats()
    full = held.cigars(extended=True)
    s1 = ss.stats()
    assert (s1["fill_ms"], s1["refill_ms"]) == (s0["fill_ms"], s0["refill_ms"]) and s1["wall_ms"] >= s1["fetch_kernel_ms"] >= 0
    assert digest(held, S, labels) == before
    INV = _ffi.ERR_INVALID_ARGUMENT
    which = np.arange(0, n, 2, dtype=np.uint32)
    rec = np.full(32 * len(which), 7, dtype=np.uint8)
    summ = _ffi.CigarSummary(9, 9, 9, 9, 9, 9, (C.c_uint32 * 3)(9, 9, 9))

    def plan(flags=0, w=which, n_w=None, r=rec, s=summ):
        return lib.aln_seqset_held_cigar_plan(ss.handle, flags, w.ctypes.data if w is not None else None, len(w) if n_w is None else n_w,
                                              r.ctypes.data if r is not None else None, C.byref(s) if s is not None else None)

    def fill(o, cap, f=None, cap_f=0):
        return lib.aln_seqset_held_cigar_fill(ss.handle, o.ctypes.data if o is not None else None, cap, f.ctypes.data if f is not None else None, cap_f)

    # two plans in a row, then the fill: the second plan's bytes; the fill twice: the same bytes
    half = held.cigars(keep=which)
    assert plan(flags=R.CLIPS) == 0 and plan() == 0 and summ.listed == len(which) and summ.total_ops == half.summary["total_ops"]
    assert rec.view(cigar.RECORD_DTYPE).tolist() == half.records.tolist()
    total = int(summ.total_ops)
    ops = np.full(total + 4, 7, dtype=np.uint32)
    off = np.full(len(which) + 3, 7, dtype=np.uint64)
    assert fill(ops, total, off, len(which) + 1) == 0
    assert ops[:total].tolist() == half.words.tolist() and (ops[total:] == 7).all() and off[:len(which) + 1].tolist() == half.offsets.tolist() and (off[-2:] == 7).all()
    again = np.full(total + 4, 7, dtype=np.uint32)
    assert fill(again, total + 4) == 0 and again.tobytes() == ops.tobytes()
    # the plan's refusals leave the records, the summary, the stats and the plan before them as they were
    stats = ss.stats()
    rec.fill(7)
    summ = _ffi.CigarSummary(9, 9, 9, 9, 9, 9, (C.c_uint32 * 3)(9, 9, 9))
    for flags in (4, 8, 0x80000000, 7):
        assert plan(flags=flags) == INV and b"flag" in lib.aln_last_error()
    assert plan(w=None, n_w=len(which)) == INV and plan(r=None) == INV and plan(s=None) == INV
    assert plan(w=np.array([0, n], dtype=np.uint32)) == INV and b"beyond" in lib.aln_last_error()
    assert plan(n_w=0x7FFFFFF1) == INV
    assert (rec == 7).all() and [getattr(summ, f[0]) for f in _ffi.CigarSummary._fields_[:-1]] == [9] * 6 and ss.stats() == stats
    # the fill's: a capacity one word short, an offsets capacity one short, a null buffer
    ops.fill(7)
    off.fill(7)
    assert fill(ops, total - 1) == INV and b"capacity" in lib.aln_last_error() and fill(ops, total, off, len(which)) == INV and fill(None, total) == INV
    assert (ops == 7).all() and (off == 7).all() and ss.stats() == stats
    assert fill(ops, total) == 0 and ops.tobytes() == again.tobytes(), "a refused plan leaves the plan before it usable"
    assert digest(held, S, labels) == before
    # a new held pass: the plan is of hits that are gone
    ss.hits(S, DEL, EXT, 150.0, None)
    ops.fill(7)
    assert fill(ops, total + 4) == INV and b"plan" in lib.aln_last_error() and (ops == 7).all()
    assert plan() == 0 and fill(ops, total) == 0 and ops.tobytes() == again.tobytes()
    assert held.cigars(extended=True).words.tobytes() == full.words.tobytes()
    # no held pass at all: a score pass replaces it; a set that never had a plan
    ss.score(S, DEL, EXT, rectangle(0, 2, 0, 2))
    ops.fill(7)
    assert plan() == INV and fill(ops, total) == INV and (ops == 7).all()
    case.held = ss.hits(S, DEL, EXT, 150.0, None)
    with SeqSet(hand_built()[:3]) as fresh:
        fresh.hits(S, DEL, EXT, 150.0, None)
        assert lib.aln_seqset_held_cigar_fill(fresh.handle, ops.ctypes.data, len(ops), None, 0) == INV and b"no plan" in lib.aln_last_error()
        assert (ops == 7).all()


# ---------------------------------------------------------------- the C99 caller, and the command
def hexd(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def test_through_c(tmp_path):
    """tests/abi_cigar.c: both exports called from C99 on buffers of exactly the documented sizes, each followed by a guard zone"""
    codes = hand_built()[:12]
    S = get_blosum62()
    with SeqSet(codes) as ss:
        case = Case(ss.hits(S, DEL, EXT, 150.0, rectangle(0, len(codes), 0, len(codes))))
        held = case.held
        which = list(range(len(held) - 1, -1, -3)) + [1, 1]
        flag_list = [0, R.EXTENDED | R.CLIPS]
        words = [len(codes)] + [len(c) for c in codes] + [int(x) for c in codes for x in c]
        words += [S.shape[0], S.shape[1]] + [hexd(x) for x in S.ravel()] + [hexd(DEL), hexd(EXT), hexd(150.0), BLANK]
        words += [len(which)] + which + [len(flag_list)] + flag_list
        path = tmp_path / "case.txt"
        path.write_text(" ".join(str(w) for w in words) + "\n")
        exe = native_build.build_cigar_harness()
        run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout[-3000:] + run.stderr
        lines = [l.split() for l in run.stdout.splitlines()]
        assert lines[-1] == ["guards", "ok"] and ["held", str(len(held))] in lines
        calls = [k for k, l in enumerate(lines) if l[:2] == ["rc", "held_cigar_plan"]]
        assert [lines[k][2:] for k in calls] == [[str(f), "0"] for f in flag_list]
        for k, flags in zip(calls, flag_list):
            recs, off, ops, summ = R.listed(case.entries, which, len(held), BLANK, flags)
            rec_line, sum_line, fill_line, off_line, ops_line = lines[k + 1:k + 6]
            assert (rec_line[0], sum_line[0], off_line[0], ops_line[0]) == ("records", "summary", "offsets", "ops")
            assert fill_line == ["rc", "held_cigar_fill", str(flags), "0"]
            flat = [int(x) for x in rec_line[1:]]
            assert [tuple(flat[i:i + 8]) for i in range(0, len(flat), 8)] == recs
            assert [int(x) for x in sum_line[1:]] == [summ[key] for key in R.SUMMARY_KEYS]
            assert [int(x) for x in off_line[1:]] == off and [int(x) for x in ops_line[1:]] == ops and len(ops) > len(which)


def parse_paf(path):
    return [l.split("\t") for l in open(path).read().splitlines()]


def test_the_command(capsys, tmp_path):
    path = str(tmp_path / "families.fasta")                            # 14 records of a few families: 91 pairs reach f = 30, 6 of them half identical
    with open(path, "w") as fh:
        for i, c in enumerate(cluster_cases.family_set()[0][:14]):
            fh.write(">s%d some words\n%s\n" % (i, Protein.vec_to_str(c)))
    records = read_fasta(path)
    heads = [r.head.decode("utf-8", "replace") for r in records]
    codes = encode_records(records, Protein)
    S = get_blosum62()
    out = str(tmp_path / "hits.paf")

    def expect(held, order, flags, rows):
        recs, off, words, summ, _ = R.from_held(held, order, flags, BLANK)
        assert len(rows) == len(order) >= 1
        for row, h, rec, a, b in zip(rows, order, recs, off, off[1:]):
            q, t = int(held.q[h]), int(held.t[h])
            assert row == [heads[q], str(len(codes[q])), str(rec[1]), str(rec[2]), "+", heads[t], str(len(codes[t])), str(rec[3]), str(rec[4]), str(rec[5]),
                           str(rec[6]), "255", "af:f:%r" % float(held.f[h]), "cg:Z:" + R.text(words[a:b])]

    with SeqSet(codes) as ss:
        for extra, flags in (([], 0), (["--eqx"], R.EXTENDED)):
            argv = ["-i", path, "--f-min", "30"]
            assert allpairs.main(argv + ["--paf", out] + extra) == 0
            with_file = capsys.readouterr().out
            assert allpairs.main(argv) == 0
            assert capsys.readouterr().out == with_file                 # the rows are what they were
            held = ss.hits(S, 11.0, 2.0, 30.0, None)
            expect(held, list(range(len(held))), flags, parse_paf(out))
            assert any("=" in row[13] for row in parse_paf(out)) == bool(flags)
        assert allpairs.main(["-i", path, "--f-min", "30", "--min-identity", "0.5", "--paf", out]) == 0
        rows = capsys.readouterr().out.splitlines()
        held = ss.hits(S, 11.0, 2.0, 30.0, None)
        kept = held.filter(S, min_identity=0.5).tolist()
        assert 0 < len(kept) < len(held) and len(rows) == len(kept)
        expect(held, kept, 0, parse_paf(out))
        assert allpairs.main(["-i", path, "--best", "2", "--paf", out, "--eqx"]) == 0
        rows = capsys.readouterr().out.splitlines()
        held = ss.best(S, 11.0, 2.0, 2, skip_self=True)
        order = [int(p) for _q, pos in held.by_query() for p in pos]
        got = parse_paf(out)
        expect(held, order, R.EXTENDED, got)
        assert len(rows) == len(got) and all(r[0] != r[5] for r in got), "no self pairs"
        assert allpairs.main(["-i", path, "--kmer", "3", "--best-candidates", "2", "--paf", out]) == 0
        assert len(parse_paf(out)) == len(capsys.readouterr().out.splitlines())
