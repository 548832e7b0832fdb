"""The profile rules without a GPU: aligner_amd/csrc/aln_profile_rules.h driven through a small C++ program and compared with
profile_ref.py on synthetic strings; the layout against numpy; the companion header include/aligner_hip_profile.h against its mirrors
(_ffi.PROFILE_EXPORTS, the ctypes classes, tests/abi_profile.c) and compiled as C99; the refusals that need no device; the command's
argument errors.  The same driver is also built as a stand-alone program with -fsanitize=address,undefined and run directly."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import profile_ref as R  # noqa: E402
from aligner_amd import _ffi, allpairs, profile  # noqa: E402
from aligner_amd import build as native_build  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLANK = 98

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "aln_profile_rules.h"
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "decide")) {         // lines `q t label_q label_t` -> kind center center_is_query
        uint32_t q, t, lq, lt;
        while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &q, &t, &lq, &lt) == 4) {
            uint32_t c = 77, cq = 77;
            const uint32_t kind = aln_profile_decide(q, t, lq, lt, &c, &cq);
            printf("%" PRIu32 " %" PRIu32 " %" PRIu32 "\n", kind, c, cq);
        }
        return 0;
    }
    if (!strcmp(argv[1], "count")) {          // `blank n_codes flags start len_c aln_len`, the centre's codes, the member's codes ->
        uint32_t blank, n_codes, flags, start, len_c, aln_len;      // columns seed matched deleted overflow, then the profile
        while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &blank, &n_codes, &flags, &start, &len_c, &aln_len) == 6) {
            std::vector<uint8_t> cs(aln_len), ms(aln_len);          // (exactly aln_len bytes each: a read beyond them is the sanitizer's)
            for (uint32_t j = 0; j < 2 * aln_len; ++j) {
                unsigned v;
                if (scanf("%u", &v) != 1) return 3;
                (j < aln_len ? cs[j] : ms[j - aln_len]) = (uint8_t)v;
            }
            std::vector<uint32_t> prof((size_t)aln_profile_rows(n_codes) * len_c, 0u);
            const aln_profile_tally a = aln_profile_count(cs.data(), ms.data(), aln_len, start, flags, blank, n_codes, len_c, prof.data());
            printf("%" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu64, aln_report_columns(aln_len, flags), aln_profile_seed_column(aln_len, flags),
                   a.matched, a.deleted, a.overflow);
            for (uint32_t v : prof) printf(" %" PRIu32, v);
            printf("\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "layout")) {         // `n_seqs len[] n_codes n_centers centers[]` -> centers_ok codes_ok total offsets[]
        uint64_t n;
        while (scanf("%" SCNu64, &n) == 1) {
            std::vector<uint32_t> len(n);
            for (auto &v : len) if (scanf("%" SCNu32, &v) != 1) return 3;
            uint32_t n_codes;
            uint64_t nc;
            if (scanf("%" SCNu32 " %" SCNu64, &n_codes, &nc) != 2) return 3;
            std::vector<uint32_t> cen(nc);
            for (auto &v : cen) if (scanf("%" SCNu32, &v) != 1) return 3;
            const bool ok = aln_profile_centers_ok(cen.data(), nc, n);
            printf("%d %d", (int)ok, (int)aln_profile_codes_ok(n_codes));
            if (ok) {
                std::vector<uint64_t> off(nc);
                printf(" %" PRIu64, aln_profile_layout(len.data(), cen.data(), nc, n_codes, off.data()));
                for (uint64_t v : off) printf(" %" PRIu64, v);
            }
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
    return build_driver(tmp_path_factory.mktemp("profile_rules"))


def run(drv, what, lines):
    out = subprocess.run([drv, what], capture_output=True, text=True, input="\n".join(lines) + "\n", timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.splitlines()


# ---------------------------------------------------------------- who counts
KINDS = {0: R.COUNTS, 1: R.SELF, 2: R.BETWEEN, 4: R.SKIP}


def decide_cases():
    labels = [0, 1, 2, 5, 9, R.NONE, 0xFFFFFFF0]
    nodes = [0, 1, 2, 5, 9]
    return [(q, t, lq, lt) for q in nodes for t in nodes for lq in labels for lt in labels]


def check_decide(drv):
    cases = decide_cases()
    out = run(drv, "decide", ["%d %d %d %d" % c for c in cases])
    assert len(out) == len(cases)
    seen = set()
    for (q, t, lq, lt), line in zip(cases, out):
        kind, c, cq = [int(x) for x in line.split()]
        label = {q: lq, t: lt}
        if q == t and lq != lt:
            continue                                              # (one sequence has one label)
        want, centre = R.kind_of(q, t, label, {q, t})             # every centre listed: UNLISTED is the caller's
        assert KINDS[kind] == want, (q, t, lq, lt)
        seen.add(kind)
        if want == R.COUNTS:
            assert c == centre and cq == int(q == centre)
        else:
            assert (c, cq) == (77, 77)                            # untouched
    assert seen == {0, 1, 2, 4}


def test_who_counts(driver):
    check_decide(driver)
    # with a centre that is not listed, the reference says unlisted where the header says counts
    assert R.kind_of(3, 4, {3: 3, 4: 3}, {}) == (R.UNLISTED, 3) and R.kind_of(4, 3, {3: 3, 4: 3}, {3: 0}) == (R.COUNTS, 3)


# ---------------------------------------------------------------- columns, positions and rows on synthetic strings
def synthetic(rng, aln_len, n_codes, blank):
    """two aligned strings with blanks on both sides, residues below, at and beyond n_codes"""
    pool = list(range(n_codes)) + [n_codes, n_codes + 1, 200, 255]
    pool = [x for x in pool if x != blank and x < 256]
    cs = rng.choice(pool, size=aln_len)
    ms = rng.choice(pool, size=aln_len)
    where = rng.random(aln_len)
    cs[where < 0.2] = blank
    ms[(where >= 0.2) & (where < 0.4)] = blank
    both = rng.random(aln_len) < 0.03
    cs[both] = blank
    ms[both] = blank
    return cs.astype(np.uint8), ms.astype(np.uint8)


def count_cases():
    rng = np.random.default_rng(1807)
    cases = []
    for aln_len in list(range(0, 70)) + [126, 127, 128, 129, 130, 191, 192, 193, 199, 200]:
        for flags in (0, 1):
            n_codes = int(rng.choice([1, 4, 20, 24, 63, 64]))
            cs, ms = synthetic(rng, aln_len, n_codes, BLANK)
            residues = int((cs != BLANK).sum())
            start = int(rng.integers(0, 40))
            # the centre: long enough, exactly long enough, or too short by a few (the overflow counter)
            len_c = max(0, start + residues + int(rng.choice([5, 0, 0, -1, -3])))
            cases.append((BLANK, n_codes, flags, start, len_c, aln_len, cs, ms))
    # a blank code below n_codes is a residue row for the member and still a blank for the centre; all blank; no blank at all
    cs, ms = synthetic(rng, 90, 20, 7)
    cases.append((7, 20, 0, 3, 100, 90, cs, ms))
    cases.append((BLANK, 20, 1, 0, 10, 30, np.full(30, BLANK, dtype=np.uint8), np.arange(30, dtype=np.uint8)))
    cases.append((BLANK, 20, 0, 2, 70, 65, (np.arange(65) % 20).astype(np.uint8), (np.arange(65) % 23).astype(np.uint8)))
    return cases


def check_count(drv):
    cases = count_cases()
    lines = ["%d %d %d %d %d %d %s %s" % (b, nc, fl, st, lc, n, " ".join(str(x) for x in cs), " ".join(str(x) for x in ms))
             for b, nc, fl, st, lc, n, cs, ms in cases]
    out = run(drv, "count", lines)
    assert len(out) == len(cases)
    overflowed = seeds = 0
    for (blank, n_codes, flags, start, len_c, aln_len, cs, ms), line in zip(cases, out):
        got = [int(x) for x in line.split()]
        summary = dict(status=0, aln_len=aln_len, start_x=start, start_y=12345)
        want, rec, summ = R.profiles([0], [1], [summary], [(cs, ms)], [0, 0], [0], [len_c, 1], n_codes, blank, flags)
        assert got[0] == R.counted_columns(aln_len, flags)
        assert got[1] == (0xFFFFFFFF if flags or aln_len == 0 else aln_len - 1)
        assert tuple(got[2:4]) == rec[0][2:4] and got[4] == summ["overflow"]
        assert got[5:] == want.tolist()
        assert int(want.sum()) + summ["overflow"] == int((cs[:got[0]] != blank).sum())          # one count per centre residue
        overflowed += summ["overflow"] > 0
        seeds += flags == 0 and aln_len > 0 and cs[aln_len - 1] != blank
        # the centre as the target: the same strings the other way round, the other start coordinate
        summary = dict(status=0, aln_len=aln_len, start_x=54321, start_y=start)
        other, rec_t, summ_t = R.profiles([1], [0], [summary], [(ms, cs)], [0, 0], [0], [len_c, 1], n_codes, blank, flags)
        assert other.tolist() == want.tolist() and rec_t == rec and summ_t == summ
    assert overflowed >= 5 and seeds >= 20


def test_columns_positions_and_rows(driver):
    check_count(driver)


def test_the_seed_column_sits_on_the_end_residue():
    """the traceback's last column repeats the end cell's pair: counted, it lands where the column before it landed"""
    centre = np.array([3, 4, 5, 5], dtype=np.uint8)              # residues 10, 11, 12 of the centre, then the seed: residue 12 again
    member = np.array([3, BLANK, 6, 6], dtype=np.uint8)
    s = dict(status=0, aln_len=4, start_x=10, start_y=0)
    on, _r, so = R.profiles([0], [1], [s], [(centre, member)], [0, 0], [0], [13, 9], 20, BLANK, 1)
    off, _r, sf = R.profiles([0], [1], [s], [(centre, member)], [0, 0], [0], [13, 9], 20, BLANK, 0)
    assert so["overflow"] == sf["overflow"] == 0
    on, off = on.reshape(22, 13), off.reshape(22, 13)
    assert on[3, 10] == 1 and on[20, 11] == 1 and on[6, 12] == 1 and on.sum() == 3
    assert off[6, 12] == 2 and off.sum() == 4 and (off - on).sum() == 1
    assert R.positions([BLANK, 7], 5, 2, 0, BLANK) == [(1, 5)]     # a seed with no residue in front of it stays at start


# ---------------------------------------------------------------- the layout
def layout_cases():
    rng = np.random.default_rng(3)
    cases = []
    for n in (1, 2, 7, 40):
        lens = rng.integers(0, 300, size=n)
        for k in sorted({0, 1, n // 2, n}):
            cen = np.sort(rng.choice(n, size=k, replace=False))
            cases.append((lens.tolist(), int(rng.choice([1, 20, 64])), cen.tolist()))
    cases.append(([5, 6, 7], 20, [1, 1]))            # not strictly ascending
    cases.append(([5, 6, 7], 20, [2, 1]))
    cases.append(([5, 6, 7], 20, [0, 3]))            # beyond the set
    cases.append(([5, 6, 7], 0, [0]))                # n_codes outside 1 .. 64
    cases.append(([5, 6, 7], 65, [0]))
    cases.append(([0x7FFFFFF0] * 3, 64, [0, 1, 2]))  # 64-bit totals
    return cases


def check_layout(drv):
    cases = layout_cases()
    out = run(drv, "layout", ["%d %s %d %d %s" % (len(l), " ".join(map(str, l)), nc, len(c), " ".join(map(str, c))) for l, nc, c in cases])
    assert len(out) == len(cases)
    for (lens, n_codes, cen), line in zip(cases, out):
        got = [int(x) for x in line.split()]
        ascending = all(c < len(lens) for c in cen) and all(a < b for a, b in zip(cen, cen[1:]))
        assert got[0] == int(ascending) and got[1] == int(1 <= n_codes <= 64)
        if ascending:
            off, total = R.layout(lens, cen, n_codes)
            assert got[2] == total and got[3:] == off
            np_off, np_total = profile.layout(lens, np.array(cen, dtype=np.uint32), n_codes)
            assert np_total == total == (n_codes + 2) * sum(lens[c] for c in cen) and np_off.tolist() == off


def test_layout_offsets(driver):
    check_layout(driver)


def test_the_driver_under_sanitizers(tmp_path):
    """the same three checks with the driver built as a stand-alone program under AddressSanitizer and UBSan (host code only)"""
    try:
        exe = build_driver(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    except subprocess.CalledProcessError:
        print("no sanitizer runtime for this compiler: the plain driver's tests stand alone")
        return
    check_decide(exe)
    check_count(exe)
    check_layout(exe)


def test_default_centers_and_frequency():
    lab = np.array([0, 0, 2, 5, 5, 5, R.NONE, 7, 9, 9], dtype=np.uint32)      # 8 and 9: label 9 is a member's own number
    assert profile.default_centers(lab).tolist() == [0, 5, 9]
    assert profile.default_centers(np.zeros(0, dtype=np.uint32)).tolist() == []
    assert profile.default_centers(np.array([R.NONE, 1], dtype=np.uint32)).tolist() == []
    lens = np.array([3, 4], dtype=np.uint64)
    out = np.arange(6 * 4, dtype=np.uint32)
    own = np.array([1, 3, 0, 9], dtype=np.uint8)
    p = profile.Profiles(np.array([1], dtype=np.uint32), lens, lambda i: own, 4, out, np.zeros(1, dtype=profile.RECORD_DTYPE), {})
    assert p.counts(0).shape == (6, 4) and p.counts(0)[5, 3] == 23
    f = p.frequency(0)
    assert f.dtype == np.float64 and f.shape == (4, 4)
    want = out.reshape(6, 4)[:4].astype(np.float64)
    assert (p.frequency(0, with_center=False) == want).all()
    want[1, 0] += 1
    want[3, 1] += 1
    want[0, 2] += 1                                                 # (code 9 is beyond n_codes: nothing)
    assert (f == want).all()


# ---------------------------------------------------------------- the companion header and its mirrors
def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared(path):
    return sorted(set(re.findall(r"\b(aln_[a-z_0-9]+)\s*\(", strip_comments(open(path).read()))))


def test_the_companion_header_declares_the_profile_exports():
    assert declared(os.path.join(ROOT, "include", "aligner_hip_profile.h")) == sorted(_ffi.PROFILE_EXPORTS)
    assert len(declared(os.path.join(ROOT, "include", "aligner_hip.h"))) == 61         # the main header is as it was
    for other in (_ffi.EXPORTS, _ffi.CLUSTER_EXPORTS, _ffi.PREFILTER_EXPORTS, _ffi.SEARCH_EXPORTS):
        assert not set(_ffi.PROFILE_EXPORTS) & set(other)
    assert "aln_profile.hip" in native_build.SOURCES and "aln_profile_rules.h" in native_build.HEADERS


def test_the_library_exports_them_with_argtypes():
    native_build.build()
    lib = _ffi.load()
    for sym in _ffi.PROFILE_EXPORTS:
        fn = getattr(lib, sym)
        assert fn.argtypes is not None and fn.restype is C.c_int, sym
    assert lib.aln_abi_version() == 2


def test_every_export_is_called_from_c99():
    src = strip_comments(open(os.path.join(ROOT, "tests", "abi_profile.c")).read())
    for sym in _ffi.PROFILE_EXPORTS:
        assert re.search(r"\b%s\s*\(" % sym, src), sym


def test_the_header_compiles_as_c99_and_the_layouts_match(tmp_path):
    native_build.build()
    src = str(tmp_path / "only.c")
    with open(src, "w") as fh:
        fh.write('#include "aligner_hip_profile.h"\nint main(void) { return (int)sizeof(aln_profile_record) - 16; }\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                           str(tmp_path / "only.o")])
    exe = native_build.build_profile_harness()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("layout ")]
    assert [l[1] for l in lines] == ["aln_profile_record", "aln_profile_summary"]
    for l, cls in zip(lines, (_ffi.ProfileRecord, _ffi.ProfileSummary)):
        assert int(l[2]) == C.sizeof(cls)
        fields = [(l[k], int(l[k + 1]), int(l[k + 2])) for k in range(3, len(l), 3)]
        assert fields == [(name, getattr(cls, name).offset, getattr(cls, name).size) for name, _t in cls._fields_]
    assert C.sizeof(_ffi.ProfileRecord) == 16 and C.sizeof(_ffi.ProfileSummary) == 48
    assert profile.RECORD_DTYPE.itemsize == 16 and list(profile.RECORD_DTYPE.names) == [f[0] for f in _ffi.ProfileRecord._fields_]
    assert list(profile.SUMMARY_KEYS) == [f[0] for f in _ffi.ProfileSummary._fields_][:-1] == list(R.SUMMARY_KEYS)
    assert _ffi.PROFILE_SKIP_SEED == _ffi.REPORT_SKIP_SEED == R.SKIP_SEED and _ffi.PROFILE_MAX_CODES == 64 and R.NONE == _ffi.CLUSTER_NONE


# ---------------------------------------------------------------- refusals that need no device, and the command's argument errors
def test_refusals_without_a_device():
    native_build.build()
    lib = _ffi.load()
    INV = _ffi.ERR_INVALID_ARGUMENT
    out = (C.c_uint32 * 4)(7, 7, 7, 7)
    rec = (_ffi.ProfileRecord * 1)(_ffi.ProfileRecord(7, 7, 7, 7))
    label = (C.c_uint32 * 2)(0, 0)
    cen = (C.c_uint32 * 1)(0)
    summ = _ffi.ProfileSummary(9, 9, 9, 9, 9, 9, 9, 9)
    total = C.c_uint64(9)
    # a null set
    assert lib.aln_seqset_profile_elements(None, cen, 1, 20, C.byref(total)) == INV and total.value == 9
    assert lib.aln_seqset_held_profiles(None, None, 1, None, label, cen, 1, 20, out, 4, rec, C.byref(summ)) == INV
    assert lib.aln_seqset_held_profiles(None, None, 1, None, None, None, 0, 0, None, 0, None, None) == INV
    assert list(out) == [7] * 4 and (rec[0].center, rec[0].hits, rec[0].matched, rec[0].deleted) == (7,) * 4
    assert [getattr(summ, f[0]) for f in _ffi.ProfileSummary._fields_] == [9] * 8
    for bad in (0, 65, -1):
        with pytest.raises(ValueError):
            profile.check_codes(bad)
    assert profile.check_codes(1) == 1 and profile.check_codes(64) == 64


def test_the_commands_argument_errors(capsys):
    path = os.path.join(ROOT, "tests", "golden", "protein.fasta")
    for bad in (["--profiles", "x.txt"], ["--f-min", "30", "--profiles", "x.txt"], ["--best", "3", "--report", "--profiles", "x.txt"],
                ["--profiles"], ["--f-min", "30", "--cluster", "greedy", "--profiles"]):
        with pytest.raises(SystemExit) as e:
            allpairs.main(["-i", path] + bad)
        assert e.value.code == 2
    assert "--cluster" in capsys.readouterr().err
    assert not os.path.exists("x.txt")
