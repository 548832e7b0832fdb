"""The family-alignment rules without a GPU: aligner_amd/csrc/aln_msa_rules.h driven through a small C++ program and compared with
msa_ref.py on constructed string pairs, with the properties of a family alignment asserted from msa_ref alone; the companion header
include/aligner_hip_msa.h against its mirrors (_ffi.MSA_EXPORTS, the ctypes classes, tests/abi_msa.c) and compiled as C99; the refusals
that need no device; the command's argument errors.  The same driver is also built as a stand-alone program with
-fsanitize=address,undefined and run directly."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import msa_ref as R  # noqa: E402
from aligner_amd import _ffi, allpairs, msa  # noqa: E402
from aligner_amd import build as native_build  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLANK = 98
SEED = 77                     # the code of the constructed seed column: no residue of any case

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "aln_msa_rules.h"
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "family")) {         // `blank len_c residues[] hits`, per hit `start aln_len centre[] member[]` ->
        uint32_t blank, len_c, hits;          // overflow width ins[len_c + 1] col[len_c + 1] then the (hits + 1) x width matrix
        while (scanf("%" SCNu32 " %" SCNu32, &blank, &len_c) == 2) {
            std::vector<uint8_t> own(len_c);
            for (auto &v : own) { unsigned x; if (scanf("%u", &x) != 1) return 3; v = (uint8_t)x; }
            if (scanf("%" SCNu32, &hits) != 1) return 3;
            std::vector<uint32_t> start(hits), aln_len(hits);
            std::vector<std::vector<uint8_t>> cs(hits), ms(hits);      // (exactly aln_len bytes each: a read beyond them is the sanitizer's)
            for (uint32_t h = 0; h < hits; ++h) {
                if (scanf("%" SCNu32 " %" SCNu32, &start[h], &aln_len[h]) != 2) return 3;
                cs[h].resize(aln_len[h]); ms[h].resize(aln_len[h]);
                for (uint32_t j = 0; j < 2 * aln_len[h]; ++j) {
                    unsigned x;
                    if (scanf("%u", &x) != 1) return 3;
                    (j < aln_len[h] ? cs[h][j] : ms[h][j - aln_len[h]]) = (uint8_t)x;
                }
            }
            std::vector<uint32_t> ins(len_c + 1u, 0u), col(len_c + 1u, 0u);
            uint64_t overflow = 0;
            for (uint32_t h = 0; h < hits; ++h) overflow += aln_msa_measure(cs[h].data(), aln_len[h], start[h], blank, len_c, ins.data());
            const uint64_t width = aln_msa_layout(ins.data(), len_c, col.data());
            std::vector<uint8_t> out((size_t)(hits + 1u) * width, (uint8_t)blank);
            aln_msa_center_row(own.data(), len_c, col.data(), out.data(), width);
            for (uint32_t h = 0; h < hits; ++h)
                aln_msa_member_row(cs[h].data(), ms[h].data(), aln_len[h], start[h], blank, len_c, ins.data(), col.data(), out.data() + (size_t)(h + 1u) * width, width);
            printf("%" PRIu64 " %" PRIu64, overflow, width);
            for (uint32_t v : ins) printf(" %" PRIu32, v);
            for (uint32_t v : col) printf(" %" PRIu32, v);
            for (uint8_t v : out) printf(" %u", (unsigned)v);
            printf("\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "offsets")) {        // `n`, per record `rows width` -> ok bytes total_rows byte_off[] row_off[]
        uint64_t n;
        while (scanf("%" SCNu64, &n) == 1) {
            std::vector<aln_msa_record> rec(n);
            for (auto &r : rec) { r.center = 0; r.inserted = 0; if (scanf("%" SCNu32 " %" SCNu32, &r.rows, &r.width) != 2) return 3; }
            std::vector<uint64_t> b(n), r(n);
            uint64_t bytes = 0, rows = 0;
            const bool ok = aln_msa_offsets(rec.data(), n, b.data(), r.data(), &bytes, &rows);
            printf("%d %" PRIu64 " %" PRIu64, (int)ok, bytes, rows);
            if (ok) { for (uint64_t v : b) printf(" %" PRIu64, v); for (uint64_t v : r) printf(" %" PRIu64, v); }
            printf("\n");
        }
        return 0;
    }
    return 2;
}
"""


def build_driver(tmp, extra=()):
    cxx = os.environ.get("CXX", "g++")
    src = os.path.join(str(tmp), "drv.cpp")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(str(tmp), "drv" + ("_san" if extra else ""))
    subprocess.check_call([cxx, "-O1" if extra else "-O2", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "aligner_amd", "csrc"),
                           src, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("msa_rules"))


def run(drv, what, lines):
    out = subprocess.run([drv, what], capture_output=True, text=True, input="\n".join(lines) + "\n", timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.splitlines()


# ---------------------------------------------------------------- constructed string pairs
def hit(centre, start, script, rng):
    """One hit of `centre` from centre position `start` on.  script: a list of ('m', n) n aligned pairs, ('d', n) n centre residues
    against blanks, ('i', n) n member residues against blanks.  Returns (centre string, member string, the member's residues,
    start); the strings end with the seed column."""
    cs, ms, p = [], [], start
    for op, n in script:
        for _ in range(n):
            if op == "i":
                cs.append(BLANK)
                ms.append(int(rng.integers(0, 20)))
            else:
                cs.append(int(centre[p]))
                ms.append(BLANK if op == "d" else int(rng.integers(0, 20)))
                p += 1
    member = np.array([x for x in ms if x != BLANK], dtype=np.uint8)
    return np.array(cs + [SEED], dtype=np.uint8), np.array(ms + [SEED], dtype=np.uint8), member, start


def cases():
    rng = np.random.default_rng(1901)
    c10 = rng.integers(0, 20, size=10).astype(np.uint8)
    c40 = rng.integers(0, 20, size=40).astype(np.uint8)
    out = {}
    out["no insert"] = (c10, [[("m", 4), ("d", 2), ("m", 3)], [("m", 10)]], [1, 0])
    # global strings: the member overhangs the centre at both ends
    out["inserts before 0 and after the last residue"] = (c10, [[("i", 3), ("m", 10), ("i", 2)], [("i", 1), ("m", 4), ("d", 1), ("m", 5), ("i", 4)]], [0, 0])
    out["runs of different lengths at one position"] = (c10, [[("m", 5), ("i", 2), ("m", 4)], [("m", 3), ("i", 5), ("m", 5)], [("m", 2), ("i", 1), ("m", 2)],
                                                              [("m", 4), ("i", 1), ("m", 1), ("i", 3), ("m", 2)]], [1, 2, 3, 0])
    out["a run of 70 columns"] = (c40, [[("m", 30), ("i", 70), ("m", 10)], [("m", 12), ("i", 3), ("m", 6)], [("m", 1), ("i", 64), ("m", 2), ("i", 65), ("m", 1)]],
                                  [0, 18, 29])
    out["an insert first, local"] = (c40, [[("i", 2), ("m", 6)], [("m", 6), ("i", 2)], [("d", 2), ("m", 3), ("d", 1)]], [7, 1, 30])
    return out


def as_set(centre, scripts, starts, rng, centre_is_query=True):
    """a set of the centre (sequence 0) and one member per script, and the held list of their hits"""
    hits = [hit(centre, s, sc, rng) for sc, s in zip(scripts, starts)]
    seqs = [centre] + [h[2] for h in hits]
    n = len(hits)
    q = [0] * n if centre_is_query else list(range(1, n + 1))
    t = list(range(1, n + 1)) if centre_is_query else [0] * n
    summaries = [dict(status=0, aln_len=len(h[0]), start_x=h[3] if centre_is_query else 0, start_y=0 if centre_is_query else h[3]) for h in hits]
    strings = [(h[0], h[1]) if centre_is_query else (h[1], h[0]) for h in hits]
    return seqs, q, t, summaries, strings, hits


def driver_line(centre, hits, len_c=None):
    words = [BLANK, len(centre) if len_c is None else len_c] + [int(x) for x in centre[:len(centre) if len_c is None else len_c]] + [len(hits)]
    for cs, ms, _member, start in hits:
        words += [start, len(cs)] + [int(x) for x in cs] + [int(x) for x in ms]
    return " ".join(str(w) for w in words)


def check_cases(drv):
    all_cases = cases()
    lines, wants = [], []
    for name, (centre, scripts, starts) in all_cases.items():
        for centre_is_query in (True, False):
            rng = np.random.default_rng(7)
            seqs, q, t, summaries, strings, hits = as_set(centre, scripts, starts, rng, centre_is_query)
            mats, lists, recs, summ = R.alignments(q, t, summaries, strings, [0] * len(seqs), [0], [len(s) for s in seqs], seqs, BLANK)
            assert summ["overflow"] == 0 and summ["contributing"] == len(hits) and lists[0] == [R.NONE] + list(range(len(hits))), name
            R.check_properties(mats, lists, recs, q, t, summaries, strings, seqs, BLANK)
            assert not (mats[0] == SEED).any(), "the seed column is in the strings and not in the result"
            assert all(int(s[0][-1]) == SEED for s in strings)
            lines.append(driver_line(centre, hits))
            wants.append((mats[0], recs[0], summ))
    # what the names promise, from the reference
    m, rec, _s = wants[0]
    assert rec[3] == 0 and m.shape == (3, 10)
    m, rec, _s = wants[2]
    assert rec[2] == 10 + 3 + 4 and (m[0, :3] == BLANK).all() and (m[0, -4:] == BLANK).all() and (m[1, :3] != BLANK).all() and (m[2, :3] != BLANK).tolist() == [True, False, False]
    m, rec, _s = wants[4]
    assert rec[3] == 1 + 5 + 2                 # before position 4: 1; before 5: max(5, 1, 3); before 6: 2
    m, rec, _s = wants[6]
    assert rec[3] == 70 + 65 and m.shape[1] > 128       # before position 30: max(70, 3, 64); before 32: 65
    out = run(drv, "family", lines)
    assert len(out) == len(lines)
    for line, (m, rec, summ) in zip(out, wants):
        got = [int(x) for x in line.split()]
        len_c = rec[2] - rec[3]
        assert got[0] == 0 and got[1] == rec[2]
        ins, col = got[2:3 + len_c], got[3 + len_c:4 + 2 * len_c]
        assert R.columns(ins) == col and col[len_c] == rec[2] and sum(ins) == rec[3]
        assert got[4 + 2 * len_c:] == m.ravel().tolist()
    # a centre shorter than its strings say: overflow columns are counted and nothing is written beyond the width
    centre, scripts, starts = all_cases["inserts before 0 and after the last residue"]
    rng = np.random.default_rng(7)
    seqs, q, t, summaries, strings, hits = as_set(centre, scripts, starts, rng)
    short = [7] + [len(s) for s in seqs[1:]]
    mats, lists, recs, summ = R.alignments(q, t, summaries, strings, [0] * len(seqs), [0], short, [centre[:7]] + seqs[1:], BLANK)
    assert summ["overflow"] == (3 + 2) + (3 + 4)        # residues 7 .. 9 and the insert after residue 9, of both hits
    got = [int(x) for x in run(drv, "family", [driver_line(centre, hits, 7)])[0].split()]
    assert got[0] == summ["overflow"] and got[1] == recs[0][2] and got[4 + 2 * 7:] == mats[0].ravel().tolist()


def check_offsets(drv):
    sets = [[], [(0, 5)], [(3, 7), (0, 0), (2, 11), (300, 1)], [(0xFFFFFFF0, 0xFFFFFFFF), (1, 1)], [(0xFFFFFFFF, 0xFFFFFFFF)] * 3]
    out = run(drv, "offsets", ["%d %s" % (len(s), " ".join("%d %d" % r for r in s)) for s in sets])
    for s, line in zip(sets, out):
        got = [int(x) for x in line.split()]
        sizes = [(r + 1) * w for r, w in s]
        fits = sum(sizes) < 2 ** 64
        assert got[0] == int(fits)
        if fits:
            rec = np.array([(0, r, w, 0) for r, w in s], dtype=msa.RECORD_DTYPE)
            b, r, total, rows = msa.layout(rec) if len(s) and max(sizes) < 2 ** 62 else (None, None, sum(sizes), sum(r + 1 for r, _w in s))
            assert got[1] == sum(sizes) == total and got[2] == rows
            n = len(s)
            assert got[3:3 + n] == [sum(sizes[:i]) for i in range(n)] and got[3 + n:] == [sum(x + 1 for x, _w in s[:i]) for i in range(n)]
            if b is not None:
                assert b.tolist() == got[3:3 + n] and r.tolist() == got[3 + n:]


def test_constructed_pairs(driver):
    check_cases(driver)


def test_offsets(driver):
    check_offsets(driver)


def test_the_driver_under_sanitizers(tmp_path):
    """the same checks with the driver built as a stand-alone program under AddressSanitizer and UBSan (host code only)"""
    try:
        exe = build_driver(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    except subprocess.CalledProcessError:
        print("no sanitizer runtime for this compiler: the plain driver's tests stand alone")
        return
    check_cases(exe)
    check_offsets(exe)


def test_family_alignments_views():
    rec = np.array([(4, 1, 3, 1), (9, 2, 2, 0)], dtype=msa.RECORD_DTYPE)
    out = np.array([0, BLANK, 1, 5, 6, BLANK, 2, 3, 2, BLANK, BLANK, 3], dtype=np.uint8)
    row_hit = np.array([R.NONE, 7, R.NONE, 2, 5], dtype=np.uint32)
    q = np.array([0, 0, 9, 0, 0, 1, 0, 4], dtype=np.uint32)
    t = np.array([0, 0, 8, 0, 0, 9, 0, 6], dtype=np.uint32)
    from aligner_amd.enums import Protein
    fam = msa.FamilyAlignments(np.array([4, 9], dtype=np.uint32), rec, {}, out, row_hit, q, t, Protein, BLANK)
    assert len(fam) == 2 and fam.rows(0).tolist() == [[0, BLANK, 1], [5, 6, BLANK]] and fam.rows(1).shape == (3, 2)
    assert fam.hits(0).tolist() == [7] and fam.hits(1).tolist() == [2, 5]
    assert fam.members(0).tolist() == [4, 6] and fam.members(1).tolist() == [9, 8, 1]
    text = fam.text(0)
    assert text == [Protein.vec_to_str([0]) + "-" + Protein.vec_to_str([1]), Protein.vec_to_str([5, 6]) + "-"]


# ---------------------------------------------------------------- the companion header and its mirrors
def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared(path):
    return sorted(set(re.findall(r"\b(aln_[a-z_0-9]+)\s*\(", strip_comments(open(path).read()))))


def test_the_companion_header_declares_the_msa_exports():
    assert _ffi.MSA_EXPORTS == ["aln_seqset_held_msa_fill", "aln_seqset_held_msa_plan"]
    assert declared(os.path.join(ROOT, "include", "aligner_hip_msa.h")) == sorted(_ffi.MSA_EXPORTS)
    assert len(declared(os.path.join(ROOT, "include", "aligner_hip.h"))) == 61         # the main header is as it was
    for other in (_ffi.EXPORTS, _ffi.CLUSTER_EXPORTS, _ffi.PREFILTER_EXPORTS, _ffi.SEARCH_EXPORTS, _ffi.PROFILE_EXPORTS):
        assert not set(_ffi.MSA_EXPORTS) & set(other)
    assert "aln_msa.hip" in native_build.SOURCES and "aln_msa_rules.h" in native_build.HEADERS
    assert any(h.endswith("aligner_hip_msa.h") for h in native_build.HEADERS)


def test_the_library_exports_them_with_argtypes():
    native_build.build()
    lib = _ffi.load()
    for sym in _ffi.MSA_EXPORTS:
        fn = getattr(lib, sym)
        assert fn.argtypes is not None and fn.restype is C.c_int, sym
    assert lib.aln_abi_version() == 2


def test_every_export_is_called_from_c99():
    src = strip_comments(open(os.path.join(ROOT, "tests", "abi_msa.c")).read())
    for sym in _ffi.MSA_EXPORTS:
        assert re.search(r"\b%s\s*\(" % sym, src), sym


def test_the_header_compiles_as_c99_and_the_layouts_match(tmp_path):
    native_build.build()
    src = str(tmp_path / "only.c")
    with open(src, "w") as fh:
        fh.write('#include "aligner_hip_msa.h"\nint main(void) { return (int)sizeof(aln_msa_record) - 16; }\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                           str(tmp_path / "only.o")])
    exe = native_build.build_msa_harness()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("layout ")]
    assert [l[1] for l in lines] == ["aln_msa_record", "aln_msa_summary"]
    for l, cls in zip(lines, (_ffi.MsaRecord, _ffi.MsaSummary)):
        assert int(l[2]) == C.sizeof(cls)
        fields = [(l[k], int(l[k + 1]), int(l[k + 2])) for k in range(3, len(l), 3)]
        assert fields == [(name, getattr(cls, name).offset, getattr(cls, name).size) for name, _t in cls._fields_]
    assert C.sizeof(_ffi.MsaRecord) == 16 and C.sizeof(_ffi.MsaSummary) == 48
    assert [(n, _ffi.MsaRecord.__dict__[n].offset) for n, _t in _ffi.MsaRecord._fields_] == [("center", 0), ("rows", 4), ("width", 8), ("inserted", 12)]
    assert [(n, _ffi.MsaSummary.__dict__[n].offset) for n, _t in _ffi.MsaSummary._fields_] == [
        ("held", 0), ("contributing", 8), ("self_pairs", 16), ("between_members", 20), ("unlisted", 24), ("overflow", 28), ("bytes", 32), ("total_rows", 40)]
    assert msa.RECORD_DTYPE.itemsize == 16 and list(msa.RECORD_DTYPE.names) == [f[0] for f in _ffi.MsaRecord._fields_]
    assert [msa.RECORD_DTYPE.fields[n][1] for n in msa.RECORD_DTYPE.names] == [0, 4, 8, 12]
    assert list(msa.SUMMARY_KEYS) == [f[0] for f in _ffi.MsaSummary._fields_] == list(R.SUMMARY_KEYS)
    assert R.NONE == _ffi.CLUSTER_NONE


# ---------------------------------------------------------------- refusals that need no device, and the command's argument errors
def test_refusals_without_a_device():
    native_build.build()
    lib = _ffi.load()
    INV = _ffi.ERR_INVALID_ARGUMENT
    rec = (_ffi.MsaRecord * 2)(_ffi.MsaRecord(7, 7, 7, 7), _ffi.MsaRecord(7, 7, 7, 7))
    label = (C.c_uint32 * 4)(0, 0, 2, 2)
    cen = (C.c_uint32 * 2)(0, 2)
    unsorted = (C.c_uint32 * 2)(2, 0)
    twice = (C.c_uint32 * 2)(2, 2)
    summ = _ffi.MsaSummary(9, 9, 9, 9, 9, 9, 9, 9)
    flt = _ffi.HitFilter(0.5, 0.0, 0.0, 0, 0)
    out = (C.c_uint8 * 8)(*([7] * 8))
    rows = (C.c_uint32 * 2)(7, 7)
    # a null set
    assert lib.aln_seqset_held_msa_plan(None, None, 0, None, label, cen, 2, rec, C.byref(summ)) == INV and b"null" in lib.aln_last_error()
    assert lib.aln_seqset_held_msa_plan(None, None, 0, None, None, None, 0, None, None) == INV
    # flags != 0: there is no flag
    for flags in (1, 2, 0x80000000):
        assert lib.aln_seqset_held_msa_plan(None, None, flags, None, label, cen, 2, rec, C.byref(summ)) == INV and b"flags" in lib.aln_last_error()
    # unsorted centres
    for bad in (unsorted, twice):
        assert lib.aln_seqset_held_msa_plan(None, None, 0, None, label, bad, 2, rec, C.byref(summ)) == INV and b"ascending" in lib.aln_last_error()
    assert lib.aln_seqset_held_msa_plan(None, None, 0, None, label, None, 2, rec, C.byref(summ)) == INV
    # a filter without params
    assert lib.aln_seqset_held_msa_plan(None, None, 0, C.byref(flt), label, cen, 2, rec, C.byref(summ)) == INV and b"come together" in lib.aln_last_error()
    # a fill without a plan (without a set there is none)
    assert lib.aln_seqset_held_msa_fill(None, out, 8, rows, 2) == INV
    assert lib.aln_seqset_held_msa_fill(None, None, 0, None, 0) == INV
    assert all((r.center, r.rows, r.width, r.inserted) == (7,) * 4 for r in rec) and list(out) == [7] * 8 and list(rows) == [7, 7]
    assert [getattr(summ, f[0]) for f in _ffi.MsaSummary._fields_] == [9] * 8


def test_the_commands_argument_errors(capsys):
    path = os.path.join(ROOT, "tests", "golden", "protein.fasta")
    for bad in (["--msa", "x.fa"], ["--f-min", "30", "--msa", "x.fa"], ["--best", "3", "--report", "--msa", "x.fa"], ["--msa"],
                ["--f-min", "30", "--cluster", "greedy", "--msa"]):
        with pytest.raises(SystemExit) as e:
            allpairs.main(["-i", path] + bad)
        assert e.value.code == 2
    assert "--cluster" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        allpairs.main(["-i", path, "--heuristic", "--kd", "1", "--r-squared", "0.9", "--cluster", "greedy", "--msa", "x.fa"])
    assert e.value.code == 2 and "--heuristic" in capsys.readouterr().err
    assert not os.path.exists("x.fa")
