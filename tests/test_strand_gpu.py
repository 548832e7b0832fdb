"""A sequence set on both strands on the device (include/aligner_hip_strand.h): the mirrors the kernel writes against numpy, byte for
byte; every pass of a stranded set against the same pass of a plain set of host-made 2n records, bit for bit, and against the oracle;
the prefilters' lists entry for entry; the stranded CIGARs -- records, strand records, offsets, words -- against strand_ref.py, with the
aligned strings decoded back from the original records; the two plan families one after the other; the C99 caller; the command."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cigar_ref as R  # noqa: E402
import strand_cases as K  # noqa: E402
import strand_ref as S  # noqa: E402
from aligner_amd import _ffi, allpairs, cigar  # noqa: E402
from aligner_amd import build as native_build  # noqa: E402
from aligner_amd.enums import DNA  # noqa: E402
from aligner_amd.fasta import encode_records, read_fasta  # noqa: E402
from aligner_amd.matrices import nucleotide_matrix  # noqa: E402
from aligner_amd.seqset import SeqSet, both, minus, rectangle  # noqa: E402

pytestmark = pytest.mark.gpu
BLANK = 98
ALL_FLAGS = (0, R.EXTENDED, R.CLIPS, R.EXTENDED | R.CLIPS)
INV, UNS = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


# ---------------------------------------------------------------- the mirrors
def test_mirror_residues_byte_for_byte():
    recs, table = K.mirror_records(), K.odd_table()
    n = len(recs)
    assert sorted(len(r) for r in recs) == [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
    assert set(np.concatenate(recs).tolist()) == set(range(256)) and table[table].tolist() != list(range(256))
    with SeqSet.stranded(recs, map=table) as ss:
        assert ss.records == n and len(ss) == 2 * n and ss.lib.aln_seqset_strand_records(ss.handle) == n
        assert sum(int(o) % 16 != 0 for o in ss.off[:n]) >= n - 3, "the offsets are unaligned"
        off, total, _bytes = S.layout([len(r) for r in recs])
        assert ss.off.tolist() == off and ss.len.tolist() == [len(r) for r in recs] * 2
        got = ss.residues()
        want = recs + S.mirrors_numpy(recs, table)
        assert len(got) == 2 * n
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.tobytes() == w.tobytes(), "record %d of %d residues" % (i, len(w))
        assert [x.tobytes() for x in ss.residues(n + 3, 4)] == [w.tobytes() for w in want[n + 3:n + 7]]
        assert ss.lib.aln_seqset_strand_residues(ss.handle, 2 * n, 1, ss.off.ctypes.data, got[-1].ctypes.data) == INV
        assert ss.stats()["bytes_down"] == sum(len(w) for w in want[n + 3:n + 7])
    with SeqSet(recs[:4], alphabet=DNA) as plain:
        assert plain.records == 4 == len(plain) and plain.lib.aln_seqset_strand_records(plain.handle) == 0


def test_identity_map_and_creation_refusals():
    recs = [np.arange(40, dtype=np.uint8), np.zeros(0, dtype=np.uint8), np.array([9], dtype=np.uint8)]
    with SeqSet.stranded(recs, map=np.arange(256, dtype=np.uint8)) as ss:
        assert [x.tolist() for x in ss.residues()] == [r.tolist() for r in recs] + [r[::-1].tolist() for r in recs]
        lib, ctx = ss.lib, None
        from aligner_amd import runtime
        ctx = runtime.context(None)
        st = C.c_int(0)
        one = (C.c_uint64 * 1)(0)
        table = (C.c_uint8 * 256)(*range(256))
        codes = (C.c_uint8 * 4)(1, 2, 3, 0)
        assert lib.aln_seqset_create_stranded(ctx, codes, one, one, 1, None, C.byref(st)) is None and st.value == INV and b"null" in lib.aln_last_error()
        assert lib.aln_seqset_create_stranded(ctx, codes, one, one, 2 ** 31, table, C.byref(st)) is None and st.value == INV
        assert lib.aln_seqset_create_stranded(ctx, codes, None, one, 1, table, C.byref(st)) is None and st.value == INV
        long_ = (C.c_uint64 * 1)(0x7FFFFFF1)
        assert lib.aln_seqset_create_stranded(ctx, codes, one, long_, 1, table, C.byref(st)) is None and st.value == UNS
        four = (C.c_uint64 * 1)(4)
        assert lib.aln_seqset_create_stranded(ctx, None, one, four, 1, table, C.byref(st)) is None and st.value == INV


# ---------------------------------------------------------------- parity with a plain set of host-made 2n records
def resident_records():
    recs = K.parity_records()
    return recs, recs + [K.revcomp(r) for r in recs]


@pytest.fixture(scope="module")
def sets():
    recs, resident = resident_records()
    with SeqSet.stranded(recs, DNA) as stranded, SeqSet(resident, DNA) as plain:
        yield recs, resident, stranded, plain


def schemes():
    m = nucleotide_matrix()
    return {"local_5_4_10_1": (_ffi.CORE_LOCAL, m, K.DEL, K.EXT), "global_5_4_10_1": (_ffi.CORE_GLOBAL, m, K.DEL, K.EXT),
            "local_real": (_ffi.CORE_LOCAL, m * 0.37 + 0.013, 11.3, 2.1)}


def test_the_device_made_mirrors_are_the_host_made(sets):
    recs, resident, stranded, plain = sets
    assert [x.tobytes() for x in stranded.residues()] == [np.asarray(r, dtype=np.uint8).tobytes() for r in resident] == [x.tobytes() for x in plain.residues()]
    assert stranded.seqs.tobytes() == plain.seqs.tobytes() and stranded.off.tolist() == plain.off.tolist() and stranded.len.tolist() == plain.len.tolist()


@pytest.mark.parametrize("name", list(schemes()))
def test_score_equals_the_plain_set_and_the_oracle(sets, orc, name):
    recs, resident, stranded, plain = sets
    sem, m, d, e = schemes()[name]
    n = len(recs)
    block = both(rectangle(0, n, 0, n), n)
    assert (block.t_first, block.t_count) == (0, 2 * n) and stranded.pairs(block) == 2 * n * n == plain.pairs(block)
    f, status = stranded.score(m, d, e, block, semantics=sem)
    f_p, status_p = plain.score(m, d, e, block, semantics=sem)
    assert bits(f).tobytes() == bits(f_p).tobytes() and status.tobytes() == status_p.tobytes()
    for q in range(n):
        for t in range(2 * n):
            o = orc.align(sem, resident[q], resident[t], d, e, m)
            assert status[q * 2 * n + t] == o["status"] == 0 and f[q * 2 * n + t] == o["f"], (q, t)
    f_m, status_m = stranded.score(m, d, e, minus(rectangle(0, n, 0, n), n), semantics=sem)
    assert bits(f_m).tobytes() == bits(f.reshape(n, 2 * n)[:, n:]).tobytes()


def test_hits_and_strings_equal_the_plain_set(sets, orc):
    recs, resident, stranded, plain = sets
    sem, m, d, e = schemes()["local_5_4_10_1"]
    n = len(recs)
    # a condition on the inputs, from the oracle alone: the threshold keeps a hit on each strand, the planted pair among them
    keeps = {(q, t) for q in range(n) for t in range(2 * n) if orc.align(sem, resident[q], resident[t], d, e, m)["f"] >= K.F_MIN}
    assert (K.A, n + K.B) in keeps and (K.A, K.NEAR) in keeps and any(t < n and t != q for q, t in keeps) and any(t >= n for q, t in keeps)
    block = both(rectangle(0, n, 0, n), n)
    held = stranded.hits(m, d, e, K.F_MIN, block, semantics=sem)
    res, strs = held.strings()
    held_p = plain.hits(m, d, e, K.F_MIN, block, semantics=sem)
    res_p, strs_p = held_p.strings()
    assert set(zip(held.q.tolist(), held.t.tolist())) == keeps
    for a, b in ((held.index, held_p.index), (held.q, held_p.q), (held.t, held_p.t), (bits(held.f), bits(held_p.f)), (res, res_p)):
        assert a.tobytes() == b.tobytes()
    assert [(x.tobytes(), y.tobytes()) for x, y in strs] == [(x.tobytes(), y.tobytes()) for x, y in strs_p]
    best = stranded.best(m, d, e, 3, block=block, skip_self=True, semantics=sem)
    best_p = plain.best(m, d, e, 3, block=block, skip_self=True, semantics=sem)
    assert best.index.tobytes() == best_p.index.tobytes() and bits(best.f).tobytes() == bits(best_p.f).tobytes()
    assert not (best.q == best.t).any() and ((best.q + n) == best.t).any(), "self pairs are skipped on the plus strand only"


def test_the_prefilters_lists_equal_the_plain_sets(sets):
    recs, resident, stranded, plain = sets
    n = len(recs)
    block = both(rectangle(0, n, 0, n), n)
    for k, shared in ((6, 30), (8, 20)):
        lists = []
        for ss in (stranded, plain):
            assert ss.kmer_index(k, 4).tolist() == ss.word_index(k, 4).tolist()
            a = ss.prefilter(k, 4, min_shared=shared, block=block)
            b = ss.word_join(k, 4, min_shared=shared, block=block)
            lists.append([(c.index.tobytes(), c.q.tobytes(), c.t.tobytes(), c.shared.tobytes()) for c in (a, b)])
            assert lists[-1][0] == lists[-1][1]
            assert (K.A, n + K.B) in set(zip(a.q.tolist(), a.t.tolist())) and 0 < len(a) < 2 * n * n
        assert lists[0] == lists[1]


# ---------------------------------------------------------------- stranded CIGARs
class Case:
    """a held pass over a stranded set and its reference entries, computed once and left unchanged"""

    def __init__(self, held, table):
        self.held, self.table = held, table
        o = held.owner
        self.n = o.records
        self.entries, (self.res, self.strs, self.seqs) = R.entries_of(held, BLANK)
        self.pairs = list(zip(held.q.tolist(), held.t.tolist()))
        self.originals = [[int(c) for c in s] for s in self.seqs[:self.n]]

    def check(self, which=None, flags=0):
        held = self.held
        w = list(range(len(held))) if which is None else [int(h) for h in which]
        got = held.cigars(keep=None if which is None else np.array(w, dtype=np.uint32), extended=bool(flags & R.EXTENDED), clips=bool(flags & R.CLIPS),
                          stranded=True)
        recs, strands, off, words, summ = S.listed(self.entries, self.pairs, held.owner.len, w, self.n, len(held), BLANK, flags)
        assert got.summary == summ and summ["failed"] == 0 and summ["overflow"] == 0
        assert [tuple(int(x) for x in r) for r in got.records.tolist()] == recs
        assert [tuple(int(x) for x in r)[:5] for r in got.strands.tolist()] == strands and not got.strands["reserved"].any() and not got.strands["reserved2"].any()
        assert got.offsets.tolist() == off and got.words.tolist() == words
        assert got.q_rec.tolist() == [s[0] for s in strands] and bytes(got.strand.tolist()) == bytes(s[2] for s in strands)
        for i, h in enumerate(w):
            n = R.counted_columns(int(self.res["aln_len"][h]))
            want = ([int(c) for c in self.strs[h][0][:n]], [int(c) for c in self.strs[h][1][:n]])
            assert S.decode(got.ops(i).tolist(), recs[i], strands[i], self.originals, self.table, BLANK) == want, h
            s, r = strands[i], recs[i]
            q_o, t_o = self.originals[s[0]], self.originals[s[1]]
            d_q, d_t = cigar.decode(got.ops(i), cigar.mirror(q_o, self.table) if s[3] else q_o, cigar.mirror(t_o, self.table) if s[4] else t_o,
                                    len(q_o) - r[2] if s[3] else r[1], len(t_o) - r[4] if s[4] else r[3], BLANK, reversed_target=bool(s[4]))
            assert (d_q.tolist(), d_t.tolist()) == want
        plan = held.last_cigar_plan_stats
        assert plan["bytes_up"] == 5 * len(w) and plan["bytes_down"] == 32 * len(w) + 32
        return got


@pytest.fixture(scope="module")
def cigars_local():
    recs = K.cigar_records()
    n = len(recs)
    with SeqSet.stranded(recs, DNA) as ss:
        held = ss.hits(nucleotide_matrix(), K.DEL, K.EXT, 5.0, rectangle(0, 2 * n, 0, 2 * n))
        yield ss, Case(held, DNA.complement_map())


def test_the_cigar_set_has_what_it_is_built_for(cigars_local):
    ss, case = cigars_local
    held, n = case.held, case.n
    assert len(held) > 256, "more than one tile of the offset scan"
    kinds = {(int(q >= n), int(t >= n)) for q, t in case.pairs}
    assert kinds == {(0, 0), (0, 1), (1, 0), (1, 1)}
    n_of = [R.counted_columns(int(a)) for a in case.res["aln_len"]]
    for c in K.COLUMNS:
        for kind in kinds:
            assert any(n_of[h] == c and (int(q >= n), int(t >= n)) == kind for h, (q, t) in enumerate(case.pairs)), (c, kind)
    got = case.check()
    single = [i for i in range(len(held)) if int(got.records["n_ops"][i]) == 1]
    gapped = [i for i in range(len(held)) if set(int(w) & 15 for w in got.ops(i)) >= {R.I} or set(int(w) & 15 for w in got.ops(i)) >= {R.D}]
    assert single and gapped and any(case.pairs[i][1] >= n for i in gapped), "a single run; gap runs in reversed words"
    rev = [i for i in gapped if case.pairs[i][1] >= n and int(got.records["n_ops"][i]) >= 3]
    assert any(got.ops(i).tolist() != got.ops(i).tolist()[::-1] for i in rev), "reversing changes the words"


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_every_flag_combination(cigars_local, flags):
    ss, case = cigars_local
    got = case.check(flags=flags)
    ops = set(int(w) & 15 for w in got.words)
    assert (R.S in ops) == bool(flags & R.CLIPS) and ((R.EQ in ops) == bool(flags & R.EXTENDED))
    if flags & R.CLIPS:                                   # the clips changed places: a reversed hit ends with what the plain plan begins with
        plain = case.held.cigars(extended=bool(flags & R.EXTENDED), clips=True)
        seen = 0
        for i, (q, t) in enumerate(case.pairs):
            if t >= case.n and int(plain.records["q_start"][i]) > 0:
                assert int(got.ops(i)[-1]) == (int(plain.records["q_start"][i]) << 4) | R.S == int(plain.ops(i)[0])
                seen += 1
        assert seen


def test_lists_with_a_repeat_and_a_descending_order(cigars_local):
    ss, case = cigars_local
    n_held = len(case.held)
    full = case.check()
    down = case.check(which=list(range(n_held - 1, -1, -5)) + [3, 3, n_held - 1], flags=R.EXTENDED | R.CLIPS)
    assert down.ops(len(down) - 3).tolist() == down.ops(len(down) - 2).tolist()
    assert case.check(which=[7]).ops(0).tolist() == full.ops(7).tolist()
    none = case.check(which=[])
    assert len(none) == 0 and none.offsets.tolist() == [0]


def test_global_hits_begin_and_end_with_gap_runs():
    recs = K.cigar_records()
    n = len(recs)
    with SeqSet.stranded(recs, DNA) as ss:
        held = ss.hits(nucleotide_matrix(), 4.0, 4.0, -1e300, rectangle(0, 2 * n, 0, 2 * n), semantics=_ffi.CORE_GLOBAL)
        assert len(held) == 4 * n * n
        case = Case(held, DNA.complement_map())
        first = [(int(s[0][0]) == BLANK or int(s[1][0]) == BLANK) for s in case.strs]
        last = [(int(s[0][len(s[0]) - 2]) == BLANK or int(s[1][len(s[1]) - 2]) == BLANK) for s in case.strs]
        for kind in ((0, 0), (0, 1), (1, 0), (1, 1)):
            of = [h for h, (q, t) in enumerate(case.pairs) if (int(q >= n), int(t >= n)) == kind]
            assert any(first[h] for h in of) and any(last[h] for h in of), kind
        for flags in (0, R.EXTENDED | R.CLIPS):
            got = case.check(which=list(range(0, len(held), 3)), flags=flags)
            assert R.S not in set(int(w) & 15 for w in got.words)


def test_the_two_plan_families_one_after_the_other(cigars_local):
    ss, case = cigars_local
    lib, held = ss.lib, case.held
    which = np.arange(len(held) - 1, -1, -2, dtype=np.uint32)
    before = held.cigars(keep=which, clips=True)
    stranded = held.cigars(keep=which, clips=True, stranded=True)
    after = held.cigars(keep=which, clips=True)
    for a, b in ((before.records, after.records), (before.offsets, after.offsets), (before.words, after.words)):
        assert a.tobytes() == b.tobytes()
    assert stranded.words.tobytes() != before.words.tobytes() and stranded.offsets.tobytes() == before.offsets.tobytes()
    # the last plan is the plain one: a stranded fill is refused and the plain fill still answers
    total = int(after.summary["total_ops"])
    ops = np.full(total, 7, dtype=np.uint32)
    assert lib.aln_seqset_held_strand_cigar_fill(ss.handle, ops.ctypes.data, total, None, 0) == INV and b"plan" in lib.aln_last_error() and (ops == 7).all()
    assert lib.aln_seqset_held_cigar_fill(ss.handle, ops.ctypes.data, total, None, 0) == 0 and ops.tobytes() == after.words.tobytes()
    # ... and the other way round; a refused plan leaves the plan before it intact
    rec = np.zeros(len(which), dtype=cigar.RECORD_DTYPE)
    strands = np.zeros(len(which), dtype=cigar.STRAND_DTYPE)
    summ = _ffi.CigarSummary()
    assert lib.aln_seqset_held_strand_cigar_plan(ss.handle, R.CLIPS, which.ctypes.data, len(which), rec.ctypes.data, strands.ctypes.data, C.byref(summ)) == 0
    assert rec.tobytes() == stranded.records.tobytes() and strands.tobytes() == stranded.strands.tobytes()
    ops.fill(7)
    assert lib.aln_seqset_held_cigar_fill(ss.handle, ops.ctypes.data, total, None, 0) == INV and (ops == 7).all()
    assert lib.aln_seqset_held_strand_cigar_plan(ss.handle, 4, which.ctypes.data, len(which), rec.ctypes.data, strands.ctypes.data, C.byref(summ)) == INV
    assert lib.aln_seqset_held_strand_cigar_plan(ss.handle, 0, which.ctypes.data, len(which), rec.ctypes.data, None, C.byref(summ)) == INV
    assert lib.aln_seqset_held_strand_cigar_fill(ss.handle, ops.ctypes.data, total, None, 0) == 0 and ops.tobytes() == stranded.words.tobytes()
    # a stranded plan on a plain set is refused and leaves that set's plain plan intact
    with SeqSet(K.cigar_records()[:6], DNA) as plain:
        h = plain.hits(nucleotide_matrix(), K.DEL, K.EXT, 5.0, rectangle(0, 6, 0, 6))
        got = h.cigars()
        w = np.arange(len(h), dtype=np.uint32)
        rec = np.full(len(h), 7, dtype=cigar.RECORD_DTYPE)
        strands = np.zeros(len(h), dtype=cigar.STRAND_DTYPE)
        assert lib.aln_seqset_held_strand_cigar_plan(plain.handle, 0, w.ctypes.data, len(w), rec.ctypes.data, strands.ctypes.data, C.byref(summ)) == INV
        assert b"stranded" in lib.aln_last_error() and (rec["n_ops"] == 7).all()
        ops = np.zeros(int(got.summary["total_ops"]), dtype=np.uint32)
        assert lib.aln_seqset_held_cigar_fill(plain.handle, ops.ctypes.data, len(ops), None, 0) == 0 and ops.tobytes() == got.words.tobytes()
        with pytest.raises(Exception):
            h.cigars(stranded=True)


# ---------------------------------------------------------------- the C99 caller, and the command
def hexd(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def test_through_c(tmp_path, cigars_local):
    """tests/abi_strand.c: every export called from C99 on buffers of exactly the documented sizes, each followed by a guard zone"""
    ss, case = cigars_local
    codes = K.cigar_records()
    table = DNA.complement_map()
    m = nucleotide_matrix()
    held = case.held                                      # (the C program's pass is this one: the full square of the 2n, f >= 5)
    which = list(range(len(held) - 1, -1, -7)) + [1, 1]
    flag_list = [0, R.EXTENDED | R.CLIPS]
    words = [len(codes)] + [len(c) for c in codes] + [int(x) for c in codes for x in c] + table.tolist()
    words += [m.shape[0], m.shape[1]] + [hexd(x) for x in m.ravel()] + [hexd(K.DEL), hexd(K.EXT), hexd(5.0), BLANK]
    words += [len(which)] + which + [len(flag_list)] + flag_list
    path = tmp_path / "case.txt"
    path.write_text(" ".join(str(w) for w in words) + "\n")
    exe = native_build.build_strand_harness()
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr
    lines = [l.split() for l in run.stdout.splitlines()]
    assert lines[-1] == ["guards", "ok"] and ["held", str(len(held))] in lines and ["stranded", str(len(codes))] in lines
    resident = [l for l in lines if l[0] == "residues"][0][1:]
    assert [int(x) for x in resident] == ss.seqs.tolist()
    calls = [k for k, l in enumerate(lines) if l[:2] == ["rc", "held_strand_cigar_plan"]]
    assert [lines[k][2:] for k in calls] == [[str(f), "0"] for f in flag_list]
    for k, flags in zip(calls, flag_list):
        recs, strands, off, ops, summ = S.listed(case.entries, case.pairs, ss.len, which, case.n, len(held), BLANK, flags)
        rec_line, str_line, sum_line, fill_line, off_line, ops_line = lines[k + 1:k + 7]
        assert (rec_line[0], str_line[0], sum_line[0], off_line[0], ops_line[0]) == ("records", "strands", "summary", "offsets", "ops")
        assert fill_line == ["rc", "held_strand_cigar_fill", str(flags), "0"]
        flat = [int(x) for x in rec_line[1:]]
        assert [tuple(flat[i:i + 8]) for i in range(0, len(flat), 8)] == recs
        flat = [int(x) for x in str_line[1:]]
        assert [tuple(flat[i:i + 7]) for i in range(0, len(flat), 7)] == [s + (0, 0) for s in strands]
        assert [int(x) for x in sum_line[1:]] == [summ[key] for key in R.SUMMARY_KEYS]
        assert [int(x) for x in off_line[1:]] == off and [int(x) for x in ops_line[1:]] == ops and len(ops) > len(which)


def parse_paf(path):
    return [l.split("\t") for l in open(path).read().splitlines()]


def test_the_command(capsys, tmp_path):
    heads, texts = K.command_records()
    path = str(tmp_path / "reads.fasta")
    with open(path, "w") as fh:
        for h, t in zip(heads, texts):
            fh.write(">%s\n%s\n" % (h, t))
    records = read_fasta(path)
    names = [r.head.decode("utf-8", "replace") for r in records]
    out = str(tmp_path / "hits.paf")
    # one strand, as before this option existed: the rows and lines of the plain set's held pass, strand + throughout
    assert allpairs.main(["-i", path, "--dna", "--f-min", "45", "--paf", out]) == 0
    rows = capsys.readouterr().out.splitlines()
    m = nucleotide_matrix()
    with SeqSet(encode_records(records, DNA), DNA) as ss:
        held = ss.hits(m, 11.0, 2.0, 45.0, None)
        assert len(held) >= 1 and rows == ["%s,%s,%r" % (names[int(q)], names[int(t)], float(f)) for q, t, f in zip(held.q, held.t, held.f)]
        got = held.cigars()
        assert open(out).read() == "".join(got.paf(i, names[int(held.q[i])], ss.len[held.q[i]], names[int(held.t[i])], ss.len[held.t[i]], held.f[i]) + "\n"
                                           for i in range(len(held)))
    one_strand = [float(r.split(",")[2]) for r in rows if r.split(",")[:2] == [names[1], names[4]]]
    assert len(one_strand) == 1 and one_strand[0] < 300.0, "the planted pair lies on opposite strands: one strand does not find it"
    # both strands: the planted pair once, on the minus strand, with the planted coordinates
    assert allpairs.main(["-i", path, "--dna", "--both-strands", "--f-min", "300", "--paf", out]) == 0
    rows = [r.split(",") for r in capsys.readouterr().out.splitlines()]
    assert all(len(r) == 4 and r[2] in "+-" for r in rows)
    planted = [r for r in rows if {r[0], r[1]} == {names[1], names[4]}]
    assert planted == [[names[1], names[4], "-", repr(400.0)]]
    paf = parse_paf(out)
    assert len(paf) == len(rows)
    line = [l for l in paf if l[0] == names[1] and l[5] == names[4]]
    assert line == [[names[1], "110", "0", "80", "-", names[4], "120", "15", "95", "80", "80", "255", "af:f:400.0", "cg:Z:80M"]]
    # the other passes of the command take the option too: the planted pair is record 1's best partner, on the minus strand
    assert allpairs.main(["-i", path, "--dna", "--both-strands", "--best", "1", "--paf", out, "--eqx"]) == 0
    best = [r.split(",") for r in capsys.readouterr().out.splitlines()]
    assert [names[1], "1", names[4], "-", repr(400.0)] in best and [r[2:4] for r in best if r[0] == names[4]] == [[names[1], "-"]]
    assert [l[2:5] + l[7:9] + l[13:] for l in parse_paf(out) if l[0] == names[1] and l[5] == names[4]] == [["0", "80", "-", "15", "95", "cg:Z:80="]]
    assert allpairs.main(["-i", path, "--dna", "--both-strands", "--kmer", "8", "--word-join", "--min-shared", "20", "--f-min", "300"]) == 0
    assert [names[1], names[4], "-", repr(400.0)] in [r.split(",") for r in capsys.readouterr().out.splitlines()]
    assert allpairs.main(["-i", path, "--dna", "--both-strands", "--kmer", "8", "--min-shared", "20", "--best-candidates", "2", "--report"]) == 0
    assert any(r.split(",")[:4] == [names[1], "1", names[4], "-"] for r in capsys.readouterr().out.splitlines())
