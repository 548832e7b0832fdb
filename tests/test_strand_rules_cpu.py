"""The strand rules without a GPU: aligner_amd/csrc/aln_strand_rules.h driven through a small C++ program and compared with strand_ref.py
-- the mirrors' offsets, the coordinate flips of the four (qm, tm) cases, the place of every word and the clip swap; an independent
cross-check of the rule through the existing cigar.encode on reversed and complemented strings; the companion header
include/aligner_hip_strand.h against its mirrors (_ffi.STRAND_EXPORTS, the ctypes class, tests/abi_strand.c) and compiled as C99; the
refusals that need no device; the command's argument errors."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cigar_ref as R  # noqa: E402
import strand_ref as S  # noqa: E402
from aligner_amd import _ffi, allpairs, cigar, seqset  # noqa: E402
from aligner_amd import build as native_build  # noqa: E402
from aligner_amd.enums import DNA  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLANK = 98
ALL_FLAGS = (0, R.EXTENDED, R.CLIPS, R.EXTENDED | R.CLIPS)

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "aln_strand_rules.h"
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "set")) {            // `n len[n] n_probes probe[n_probes]` -> ok bytes tiles off[2n] | record_at of every probe
        uint64_t n;
        while (scanf("%" SCNu64, &n) == 1) {
            std::vector<uint64_t> len(n), off(2 * n);
            uint64_t total = 0;
            for (uint64_t i = 0; i < n; ++i) { if (scanf("%" SCNu64, &len[i]) != 1) return 3; off[i] = total; total += len[i]; }
            for (uint64_t i = 0; i < n; ++i) off[n + i] = aln_strand_mirror_off(total, off[i]);
            printf("%d %" PRIu64 " %" PRIu64, (int)aln_strand_count_ok(n), aln_strand_buffer_bytes(total), aln_strand_tiles(total));
            for (uint64_t v : off) printf(" %" PRIu64, v);
            uint64_t probes;
            if (scanf("%" SCNu64, &probes) != 1) return 3;
            printf(" |");
            for (uint64_t k = 0; k < probes; ++k) {
                uint64_t p;
                if (scanf("%" SCNu64, &p) != 1) return 3;
                const uint64_t i = aln_strand_record_at(off.data(), n, p);
                printf(" %" PRIu64 " %" PRIu64, i, aln_strand_mirror_off(total, off[i]) + aln_strand_mirror_pos(len[i], p - off[i]));
            }
            printf("\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "count")) {          // `n` -> ok
        uint64_t n;
        while (scanf("%" SCNu64, &n) == 1) printf("%d\n", (int)aln_strand_count_ok(n));
        return 0;
    }
    if (!strcmp(argv[1], "hits")) {           // `q_seq t_seq n N M` and the plain record's eight words -> the strand record's seven
        uint32_t q, t, n, N, M;               // words, the stranded record's eight, the place of every word
        aln_cigar_record r;
        while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32
                     " %" SCNu32 " %" SCNd32, &q, &t, &n, &N, &M, &r.n_ops, &r.q_start, &r.q_end, &r.t_start, &r.t_end, &r.matches, &r.block, &r.status) == 13) {
            const aln_strand_record s = aln_strand_classify(q, t, n);
            const aln_cigar_record o = aln_strand_record_of(r, s, N, M);
            printf("%" PRIu32 " %" PRIu32 " %u %u %u %u %" PRIu32, s.q_rec, s.t_rec, (unsigned)s.strand, (unsigned)s.q_mirror, (unsigned)s.t_mirror,
                   (unsigned)s.reserved, s.reserved2);
            printf(" %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRId32, o.n_ops, o.q_start, o.q_end, o.t_start,
                   o.t_end, o.matches, o.block, o.status);
            for (uint32_t w = 0; w < r.n_ops; ++w) printf(" %" PRIu64, aln_strand_word_pos(w, r.n_ops, s.t_mirror != 0));
            printf("\n");
        }
        return 0;
    }
    return 2;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("strand_rules")
    src = os.path.join(str(tmp), "drv.cpp")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(str(tmp), "drv")
    # a stand-alone host program: AddressSanitizer and UBSan where the compiler has their runtimes
    base = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "aligner_amd", "csrc"), src, "-o", exe]
    if subprocess.call(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)
    return exe


def run(drv, what, lines):
    out = subprocess.run([drv, what], capture_output=True, text=True, input="\n".join(lines) + "\n", timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.splitlines()


def test_mirror_offsets_and_the_record_of_a_position(driver):
    sets = [[5], [0, 1, 0, 0, 2, 15, 0], [1] * 40, [4095, 4096, 4097, 0, 1], [0, 0, 3], [17, 0]]
    lines, wants = [], []
    for lens in sets:
        off, total, nbytes = S.layout(lens)
        probes = sorted(set([0, total - 1] + [o for o, n in zip(off, lens) if n] + [o + n - 1 for o, n in zip(off, lens) if n]))
        lines.append("%d %s %d %s" % (len(lens), " ".join(map(str, lens)), len(probes), " ".join(map(str, probes))))
        at = []
        for p in probes:
            i = S.record_at(off, lens, p)
            at += [i, total + off[i] + (lens[i] - 1 - (p - off[i]))]
        wants.append([1, nbytes, S.tiles(total)] + off + at)
        assert off[len(lens):] == [total + o for o in off[:len(lens)]] and nbytes == 2 * total + 256
    for line, want in zip(run(driver, "set", lines), wants):
        assert [int(x) for x in line.replace("|", "").split()] == want
    counts = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 63]
    assert [int(x) for x in run(driver, "count", [str(c) for c in counts])] == [int(S.count_ok(c)) for c in counts] == [1, 1, 1, 0, 0, 0]


def plain_records():
    """(N, M, plain record) with the edges: q_start = 0, q_end = N, one op, an empty alignment with a failed status"""
    return [(40, 50, (3, 5, 30, 7, 33, 20, 28, 0)), (40, 50, (1, 0, 40, 0, 40, 40, 40, 0)), (40, 50, (1, 0, 1, 49, 50, 1, 1, 0)),
            (40, 50, (2, 39, 40, 0, 50, 1, 50, 0)), (40, 50, (0, 0, 0, 0, 0, 0, 0, 4)), (1, 1, (1, 0, 1, 0, 1, 1, 1, 0)),
            (300, 7, (9, 17, 300, 2, 7, 3, 290, 0)), (40, 50, (0, 4, 4, 9, 9, 0, 0, 0))]


def test_the_four_cases_of_a_hit(driver):
    n = 6
    lines, wants = [], []
    for N, M, plain in plain_records():
        for qm in (0, 1):
            for tm in (0, 1):
                q, t = 2 + qm * n, 5 + tm * n
                lines.append("%d %d %d %d %d %s" % (q, t, n, N, M, " ".join(map(str, plain))))
                s = S.classify(q, t, n)
                assert s == (2, 5, S.MINUS if qm != tm else S.PLUS, qm, tm)
                rec = S.record(plain, s, N, M)
                wants.append(list(s) + [0, 0] + list(rec) + [S.word_pos(r, plain[0], bool(tm)) for r in range(plain[0])])
                # what the flips promise, from the reference alone
                assert rec[0] == plain[0] and rec[5:] == plain[5:]
                if plain[7] == 0:
                    assert rec[2] - rec[1] == plain[2] - plain[1] and rec[4] - rec[3] == plain[4] - plain[3]
                    assert (rec[1], rec[2]) == ((N - plain[2], N - plain[1]) if qm else plain[1:3])
                    assert (rec[3], rec[4]) == ((M - plain[4], M - plain[3]) if tm else plain[3:5])
                else:
                    assert rec == plain == (0, 0, 0, 0, 0, 0, 0, 4)
    assert S.record((1, 0, 40, 0, 40, 40, 40, 0), (0, 0, S.MINUS, 1, 0), 40, 50)[1:3] == (0, 40)           # q_start = 0 and q_end = N
    assert S.record((2, 39, 40, 0, 50, 1, 50, 0), (0, 0, S.PLUS, 1, 1), 40, 50)[1:5] == (0, 1, 0, 50)
    out = run(driver, "hits", lines)
    assert len(out) == len(wants)
    for line, want in zip(out, wants):
        assert [int(x) for x in line.split()] == want, line


def test_the_clips_change_places_with_the_words():
    plain = [(7 << 4) | R.S, (70 << 4) | R.M, (2 << 4) | R.I, (3 << 4) | R.M, (5 << 4) | R.S]
    assert S.words(plain, (0, 0, S.MINUS, 0, 1)) == [(5 << 4) | R.S, (3 << 4) | R.M, (2 << 4) | R.I, (70 << 4) | R.M, (7 << 4) | R.S]
    assert S.words(plain, (0, 0, S.MINUS, 1, 0)) == plain and S.words(plain, (0, 0, S.PLUS, 1, 1)) == plain[::-1]
    assert S.words([(1 << 4) | R.M], (0, 0, S.MINUS, 0, 1)) == [(1 << 4) | R.M] and S.words([], (0, 0, S.MINUS, 0, 1)) == []


def random_alignment(rng, columns):
    """two aligned strings of DNA codes with gaps on both sides, never blank in both, never starting or ending with a gap"""
    qs, ts = [], []
    for j in range(columns):
        kind = "m" if j in (0, columns - 1) else rng.choice(list("mmmmxxid"))
        a = int(rng.integers(0, 4))
        b = a if kind == "m" else (a + 1 + int(rng.integers(0, 3))) % 4
        qs.append(BLANK if kind == "d" else a)
        ts.append(BLANK if kind == "i" else b)
    return qs, ts


def test_the_rule_against_the_existing_encoder_on_reversed_strings():
    """Independent of the new rule: an alignment of (q, mirror(t)), both strings reversed and complemented, is an alignment of
    (mirror(q), t) -- along the forward target.  The existing cigar.encode on it, from N - q_end and M - t_end, gives the words and the
    target coordinates the stranded rule gives the (qm, tm) = (0, 1) hit, and with q back on its own strand, (1, 0), all of them."""
    rng = np.random.default_rng(2207)
    comp = DNA.complement_map()
    assert comp[:4].tolist() == [1, 0, 3, 2] and comp[4:].tolist() == list(range(4, 256)) and comp[comp].tolist() == list(range(256))
    table = comp.copy()
    table[BLANK] = BLANK
    for trial in range(60):
        qs, ts = random_alignment(rng, int(rng.integers(1, 150)))
        q_start, t_start, q_tail, t_tail = (int(x) for x in rng.integers(0, 9, size=4))
        q_res, t_res = sum(x != BLANK for x in qs), sum(y != BLANK for y in ts)
        N, M = q_start + q_res + q_tail, t_start + t_res + t_tail
        q_end, t_end = q_start + q_res, t_start + t_res
        for flags in ALL_FLAGS:
            plain, words, _p, over = R.encode(qs + [0], ts + [0], len(qs) + 1, 0, q_start, t_start, N, BLANK, flags)
            assert over == 0 and plain[1:5] == (q_start, q_end, t_start, t_end)
            # the (0, 1) hit by the rule
            s01 = S.classify(1, 3 + 5, 5)
            rec01, words01 = S.record(plain, s01, N, M), S.words(words, s01)
            # the reversed, complemented strings through the encoder the project already has
            rq, rt = table[np.array(qs[::-1], dtype=np.uint8)], table[np.array(ts[::-1], dtype=np.uint8)]
            g_rec, g_words, _gp, g_over = cigar.encode(rq, rt, BLANK, flags, N - q_end, M - t_end, N, 0, skip_seed=False)
            assert g_over == 0 and g_words.tolist() == words01, (trial, flags)
            assert (int(g_rec["t_start"]), int(g_rec["t_end"])) == rec01[3:5] == (M - t_end, M - t_start)
            assert (int(g_rec["matches"]), int(g_rec["block"]), int(g_rec["n_ops"])) == (rec01[5], rec01[6], rec01[0])
            # ... which is the held alignment of a (1, 0) hit: the rule flips its query back and leaves the words alone
            s10 = S.classify(1 + 5, 3, 5)
            got = tuple(int(g_rec[k]) for k in R.RECORD_KEYS)
            assert S.record(got, s10, N, M) == rec01 and rec01[1:3] == (q_start, q_end) and S.words(g_words.tolist(), s10) == words01


def test_decode_gives_the_strings_back_from_the_original_records():
    rng = np.random.default_rng(5)
    table = (np.arange(256, dtype=np.uint8) * 7 + 3).astype(np.uint8)       # a bijection that is no involution
    assert table[table].tolist() != list(range(256)) and len(set(table.tolist())) == 256
    n = 3
    originals = [[int(x) for x in rng.integers(0, 90, size=L)] for L in (40, 33, 57)]
    resident = originals + [S.mirror(o, table) for o in originals]
    for q_seq in (1, 1 + n):
        for t_seq in (2, 2 + n):
            q, t = resident[q_seq], resident[t_seq]
            start_x, start_y = 3, 5
            qs, ts, i, j = [], [], start_x, start_y
            for kind in "mmmimmdddmxmmiim":
                qs.append(BLANK if kind == "d" else q[i])
                ts.append(BLANK if kind == "i" else t[j])
                i += kind != "d"
                j += kind != "i"
            for flags in ALL_FLAGS:
                plain, words, _p, _o = R.encode(qs + [0], ts + [0], len(qs) + 1, 0, start_x, start_y, len(q), BLANK, flags)
                s = S.classify(q_seq, t_seq, n)
                rec, w = S.record(plain, s, len(q), len(t)), S.words(words, s)
                assert S.decode(w, rec, s, originals, table, BLANK) == (qs, ts)
                # the package's decode, told that the words are reversed
                held_q = cigar.mirror(originals[s[0]], table) if s[3] else originals[s[0]]
                held_t = cigar.mirror(originals[s[1]], table) if s[4] else originals[s[1]]
                d_q, d_t = cigar.decode(w, held_q, held_t, len(q) - rec[2] if s[3] else rec[1], len(t) - rec[4] if s[4] else rec[3], BLANK,
                                        reversed_target=bool(s[4]))
                assert d_q.tolist() == qs and d_t.tolist() == ts
                assert np.array_equal(np.asarray(held_q), np.asarray(q)) and np.array_equal(np.asarray(held_t), np.asarray(t))


def test_cigars_hold_and_write_the_strand():
    rec = np.zeros(2, dtype=cigar.RECORD_DTYPE)
    rec[0] = (1, 2, 62, 5, 65, 60, 60, 0)
    rec[1] = (1, 0, 9, 0, 9, 9, 9, 0)
    words = np.array([(60 << 4) | R.M, (9 << 4) | R.M], dtype=np.uint32)
    strands = np.zeros(2, dtype=cigar.STRAND_DTYPE)
    strands[0] = (4, 1, ord("-"), 0, 1, 0, 0)
    strands[1] = (0, 3, ord("+"), 1, 1, 0, 0)
    got = cigar.Cigars(np.array([0, 1], dtype=np.uint32), rec, {}, np.array([0, 1, 2], dtype=np.uint64), words, strands=strands)
    assert got.q_rec.tolist() == [4, 0] and got.t_rec.tolist() == [1, 3] and bytes(got.strand.tolist()) == b"-+"
    assert got.paf(0, "q", 70, "t", 80, 1.5) == "q\t70\t2\t62\t-\tt\t80\t5\t65\t60\t60\t255\taf:f:1.5\tcg:Z:60M"
    assert got.paf(1, "q", 9, "t", 9, 2.0).split("\t")[4] == "+"
    plain = cigar.Cigars(np.array([0, 1], dtype=np.uint32), rec, {}, np.array([0, 1, 2], dtype=np.uint64), words)
    assert plain.strand is None and plain.q_rec is None and plain.paf(0, "q", 70, "t", 80, 1.5).split("\t")[4] == "+"
    assert cigar.STRAND_DTYPE.itemsize == 16 == C.sizeof(_ffi.StrandRecord)
    assert [(k, cigar.STRAND_DTYPE.fields[k][1]) for k in cigar.STRAND_DTYPE.names] == [(k, getattr(_ffi.StrandRecord, k).offset) for k, _t in _ffi.StrandRecord._fields_]


def test_the_block_helpers():
    b = seqset.rectangle(2, 3, 0, 7)
    m = seqset.minus(b, 7)
    assert (m.q_first, m.q_count, m.t_first, m.t_count, m.upper) == (2, 3, 7, 7, 0)
    w = seqset.both(b, 7)
    assert (w.q_first, w.q_count, w.t_first, w.t_count, w.upper) == (2, 3, 0, 14, 0)
    m = seqset.minus(seqset.rectangle(0, 7, 4, 2), 7)
    assert (m.t_first, m.t_count) == (11, 2)
    for bad in (seqset.upper(0, 7), seqset.rectangle(0, 7, 1, 6), seqset.rectangle(0, 7, 0, 6)):
        with pytest.raises(ValueError):
            seqset.both(bad, 7)
    with pytest.raises(ValueError):
        seqset.minus(seqset.upper(0, 7), 7)


# ---------------------------------------------------------------- the companion header and its mirrors
def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared(path):
    return sorted(set(re.findall(r"\b(aln_[a-z_0-9]+)\s*\(", strip_comments(open(path).read()))))


def test_the_companion_header_declares_the_strand_exports():
    assert _ffi.STRAND_EXPORTS == ["aln_seqset_create_stranded", "aln_seqset_held_strand_cigar_fill", "aln_seqset_held_strand_cigar_plan",
                                   "aln_seqset_strand_records", "aln_seqset_strand_residues"]
    assert declared(os.path.join(ROOT, "include", "aligner_hip_strand.h")) == sorted(_ffi.STRAND_EXPORTS)
    assert len(declared(os.path.join(ROOT, "include", "aligner_hip.h"))) == 61         # the main header is as it was
    assert declared(os.path.join(ROOT, "include", "aligner_hip_cigar.h")) == sorted(_ffi.CIGAR_EXPORTS)
    others = [name for name in dir(_ffi) if name.endswith("EXPORTS") and name != "STRAND_EXPORTS"]
    assert len(others) >= 8                # the main header's, cluster, prefilter, wordjoin, search, profile, msa, cigar
    for name in others:
        assert not set(_ffi.STRAND_EXPORTS) & set(getattr(_ffi, name)), name
    assert "aln_strand.hip" in native_build.SOURCES and "aln_strand_rules.h" in native_build.HEADERS
    assert any(h.endswith("aligner_hip_strand.h") for h in native_build.HEADERS)
    launch = open(os.path.join(ROOT, "aligner_amd", "csrc", "aln_launch.h")).read()
    assert "aln_strand_launch_mirror" in launch


def test_the_library_exports_them_with_argtypes():
    native_build.build()
    lib = _ffi.load()
    for sym in _ffi.STRAND_EXPORTS:
        fn = getattr(lib, sym)
        assert fn.argtypes is not None, sym
    assert lib.aln_seqset_held_strand_cigar_plan.restype is C.c_int and lib.aln_seqset_strand_records.restype is C.c_uint64
    assert lib.aln_abi_version() == 2


def test_every_export_is_called_from_c99():
    src = strip_comments(open(os.path.join(ROOT, "tests", "abi_strand.c")).read())
    for sym in _ffi.STRAND_EXPORTS:
        assert re.search(r"\b%s\s*\(" % sym, src), sym


def test_the_header_compiles_as_c99_and_the_layout_matches(tmp_path):
    native_build.build()
    src = str(tmp_path / "only.c")
    with open(src, "w") as fh:
        fh.write('#include "aligner_hip_strand.h"\nint main(void) { return (int)sizeof(aln_strand_record) - 16; }\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                           str(tmp_path / "only.o")])
    exe = native_build.build_strand_harness()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("layout ")]
    assert [l[1] for l in lines] == ["aln_strand_record"]
    l, cls = lines[0], _ffi.StrandRecord
    assert int(l[2]) == C.sizeof(cls) == 16
    fields = [(l[k], int(l[k + 1]), int(l[k + 2])) for k in range(3, len(l), 3)]
    assert fields == [(name, getattr(cls, name).offset, getattr(cls, name).size) for name, _t in cls._fields_]
    assert fields == [("q_rec", 0, 4), ("t_rec", 4, 4), ("strand", 8, 1), ("q_mirror", 9, 1), ("t_mirror", 10, 1), ("reserved", 11, 1), ("reserved2", 12, 4)]


# ---------------------------------------------------------------- refusals that need no device, and the command's argument errors
def test_refusals_without_a_device():
    native_build.build()
    lib = _ffi.load()
    INV = _ffi.ERR_INVALID_ARGUMENT
    rec = (_ffi.CigarRecord * 2)(_ffi.CigarRecord(7, 7, 7, 7, 7, 7, 7, 7), _ffi.CigarRecord(7, 7, 7, 7, 7, 7, 7, 7))
    strands = (_ffi.StrandRecord * 2)(_ffi.StrandRecord(7, 7, 7, 7, 7, 7, 7), _ffi.StrandRecord(7, 7, 7, 7, 7, 7, 7))
    which = (C.c_uint32 * 2)(0, 1)
    summ = _ffi.CigarSummary(9, 9, 9, 9, 9, 9, (C.c_uint32 * 3)(9, 9, 9))
    ops = (C.c_uint32 * 4)(7, 7, 7, 7)
    off = (C.c_uint64 * 3)(7, 7, 7)
    plan = lib.aln_seqset_held_strand_cigar_plan
    assert plan(None, 0, which, 2, rec, strands, C.byref(summ)) == INV and b"null" in lib.aln_last_error()
    for flags in (4, 8, 0x80000000):
        assert plan(None, flags, which, 2, rec, strands, C.byref(summ)) == INV and b"flag" in lib.aln_last_error()
    assert plan(None, 0, None, 2, rec, strands, C.byref(summ)) == INV and b"null" in lib.aln_last_error()
    assert plan(None, 0, which, 2, None, strands, C.byref(summ)) == INV and b"null" in lib.aln_last_error()
    assert plan(None, 0, which, 2, rec, None, C.byref(summ)) == INV and b"null" in lib.aln_last_error()
    assert plan(None, 0, which, 2, rec, strands, None) == INV and b"null" in lib.aln_last_error()
    assert plan(None, 0, which, 0x7FFFFFF1, rec, strands, C.byref(summ)) == INV and b"too long" in lib.aln_last_error()
    assert lib.aln_seqset_held_strand_cigar_fill(None, ops, 4, off, 3) == INV
    assert lib.aln_seqset_strand_records(None) == 0
    assert lib.aln_seqset_strand_residues(None, 0, 0, None, None) == INV and b"null" in lib.aln_last_error()
    # a set without a context, a map or tables: nothing is created
    st = C.c_int(0)
    table = (C.c_uint8 * 256)(*range(256))
    one = (C.c_uint64 * 1)(0)
    assert lib.aln_seqset_create_stranded(None, None, one, one, 1, table, C.byref(st)) is None and st.value == INV
    assert all(tuple(getattr(r, f[0]) for f in _ffi.CigarRecord._fields_) == (7,) * 8 for r in rec) and list(ops) == [7] * 4 and list(off) == [7] * 3
    assert all(tuple(getattr(r, f[0]) for f in _ffi.StrandRecord._fields_) == (7,) * 7 for r in strands)
    assert [getattr(summ, f[0]) for f in _ffi.CigarSummary._fields_[:-1]] == [9] * 6 and list(summ.reserved) == [9] * 3


def test_the_commands_argument_errors(capsys):
    path = os.path.join(ROOT, "tests", "golden", "protein.fasta")
    for bad, word in ((["--both-strands"], "--dna"), (["--both-strands", "--f-min", "30"], "--dna"),
                      (["--dna", "--both-strands", "--f-min", "30", "--cluster", "greedy"], "not built"),
                      (["--dna", "--both-strands", "--best", "2", "--cluster", "components", "--profiles", "x.prof"], "not built"),
                      (["--dna", "--both-strands", "--f-min", "30", "--cluster", "greedy", "--msa", "x.msa"], "not built"),
                      (["--dna", "--both-strands", "--heuristic", "--kd", "1", "--r-squared", "0.9"], "not built")):
        with pytest.raises(SystemExit) as e:
            allpairs.main(["-i", path] + bad)
        assert e.value.code == 2
        assert word in capsys.readouterr().err, bad
    assert not os.path.exists("x.prof") and not os.path.exists("x.msa")


# ---------------------------------------------------------------- what the GPU tests' inputs are built for, from the oracle alone
def test_the_gpu_tests_inputs_have_what_they_are_built_for(orc):
    import strand_cases as K
    from aligner_amd.matrices import nucleotide_matrix
    m = nucleotide_matrix()
    recs = K.parity_records()
    n = len(recs)
    assert n == 12 and all(40 <= len(r) <= 300 for r in recs)
    resident = recs + [K.revcomp(r) for r in recs]
    assert sum(int(a != b) for a, b in zip(K.revcomp(recs[K.A]), recs[K.B])) == 3 and np.array_equal(K.revcomp(recs[K.PAL]), recs[K.PAL])
    f = {(q, t): orc.align(_ffi.CORE_LOCAL, resident[q], resident[t], K.DEL, K.EXT, m)["f"] for q in range(n) for t in range(2 * n)}
    keeps = {k for k, v in f.items() if v >= K.F_MIN}
    assert (K.A, n + K.B) in keeps and (K.A, K.NEAR) in keeps and (K.A, K.B) not in keeps and len(keeps) < n * n // 2
    # the CIGAR set: c columns without a gap between a prefix and the next, on every combination of strands
    c_recs = K.cigar_records()
    nc = len(c_recs)
    c_res = c_recs + [K.revcomp(r) for r in c_recs]
    for c, short, long_, rc in ((63, 2, 3, 11), (64, 3, 4, 12), (65, 4, 5, 13), (129, 6, 7, 14)):
        for q, t in ((short, long_), (short, nc + rc), (nc + rc, short), (nc + short, nc + long_)):
            o = orc.align(_ffi.CORE_LOCAL, c_res[q], c_res[t], K.DEL, K.EXT, m)
            assert len(o["qa"]) - 1 == c and o["f"] == 5.0 * c and BLANK not in o["qa"].tolist() + o["ta"].tolist(), (c, q, t)
    assert len(orc.align(_ffi.CORE_LOCAL, c_res[0], c_res[7], K.DEL, K.EXT, m)["qa"]) - 1 == 1
    first = orc.align(_ffi.CORE_GLOBAL, c_res[10], c_res[7], 4.0, 4.0, m)
    last = orc.align(_ffi.CORE_GLOBAL, c_res[2], c_res[7], 4.0, 4.0, m)
    assert int(first["qa"][0]) == BLANK and int(last["qa"][len(last["qa"]) - 2]) == BLANK
    # the command's reads: the planted pair, on the minus strand only, with the planted coordinates
    heads, texts = K.command_records()
    r = [DNA.str_to_vec(t) for t in texts]
    res = r + [K.revcomp(x) for x in r]
    o = orc.align(_ffi.CORE_LOCAL, res[1], res[6 + 4], 11.0, 2.0, m)
    assert (o["f"], o["start"], o["end"], len(o["qa"]) - 1) == (400.0, (25, 0), (105, 80), 80) and (len(r[1]), len(r[4])) == (110, 120)
    others = {(q, t): orc.align(_ffi.CORE_LOCAL, res[q], res[t], 11.0, 2.0, m)["f"] for q in range(6) for t in range(12) if q < t % 6}
    assert [k for k, v in others.items() if v >= 300.0] == [(1, 10)] and sum(v >= 45.0 for k, v in others.items() if k[1] < 6) >= 1
