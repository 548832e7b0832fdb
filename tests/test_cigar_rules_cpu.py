"""The CIGAR rules without a GPU: aligner_amd/csrc/aln_cigar_rules.h driven through a small C++ program and compared with cigar_ref.py on
constructed string pairs, with the round trip decode(encode(strings)) == strings asserted from cigar_ref alone; the host helpers of
aligner_amd/cigar.py against the same reference; the companion header include/aligner_hip_cigar.h against its mirrors
(_ffi.CIGAR_EXPORTS, the ctypes classes, tests/abi_cigar.c) and compiled as C99; the refusals that need no device; the command's
argument errors.  The same driver is also built as a stand-alone program with -fsanitize=address,undefined and run directly."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cigar_ref as R  # noqa: E402
from aligner_amd import _ffi, allpairs, cigar  # noqa: E402
from aligner_amd import build as native_build  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLANK = 98
ROUNDS = (0, 1, 63, 64, 65, 127, 128, 129, 200)
ALL_FLAGS = (0, R.EXTENDED, R.CLIPS, R.EXTENDED | R.CLIPS)

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "aln_cigar_rules.h"
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "hits")) {           // `blank flags status start_x start_y N aln_len room query[room] target[room]` ->
        uint32_t blank, flags, sx, sy, N, aln_len, room;      // the record's eight words, padded, overflow, the words written, the words
        int32_t status;
        while (scanf("%" SCNu32 " %" SCNu32 " %" SCNd32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &blank, &flags, &status, &sx, &sy, &N,
                     &aln_len, &room) == 8) {
            std::vector<uint8_t> q(room), t(room);            // (exactly `room` bytes each: a read beyond them is the sanitizer's)
            for (uint32_t j = 0; j < 2 * room; ++j) {
                unsigned x;
                if (scanf("%u", &x) != 1) return 3;
                (j < room ? q[j] : t[j - room]) = (uint8_t)x;
            }
            uint64_t padded = 0, overflow = 0;
            const aln_cigar_record r = aln_cigar_count(q.data(), t.data(), aln_len, status, sx, sy, N, blank, flags, &padded, &overflow);
            std::vector<uint32_t> ops(r.n_ops, 0xFFFFFFFFu);
            const uint64_t wrote = aln_cigar_write(q.data(), t.data(), aln_len, r, N, blank, flags, ops.data(), ops.size());
            printf("%" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRId32 " %" PRIu64 " %" PRIu64 " %" PRIu64,
                   r.n_ops, r.q_start, r.q_end, r.t_start, r.t_end, r.matches, r.block, r.status, padded, overflow, wrote);
            for (uint32_t w : ops) printf(" %" PRIu32, w);
            printf("\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "offsets")) {        // `n n_ops[n]` -> total off[n + 1]
        uint64_t n;
        while (scanf("%" SCNu64, &n) == 1) {
            std::vector<aln_cigar_record> rec(n, aln_cigar_empty(ALN_OK));
            for (auto &r : rec) if (scanf("%" SCNu32, &r.n_ops) != 1) return 3;
            std::vector<uint64_t> off(n + 1);
            printf("%" PRIu64, aln_cigar_offsets(rec.data(), n, off.data()));
            for (uint64_t v : off) printf(" %" PRIu64, v);
            printf("\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "limits")) {         // `max_len flags` -> supported flags_ok tiles(max_len)
        uint64_t max_len;
        uint32_t flags;
        while (scanf("%" SCNu64 " %" SCNu32, &max_len, &flags) == 2)
            printf("%d %d %" PRIu64 "\n", (int)aln_cigar_supported(max_len), (int)aln_cigar_flags_ok(flags), aln_cigar_tiles(max_len));
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
    return build_driver(tmp_path_factory.mktemp("cigar_rules"))


def run(drv, what, lines):
    out = subprocess.run([drv, what], capture_output=True, text=True, input="\n".join(lines) + "\n", timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.splitlines()


# ---------------------------------------------------------------- constructed string pairs
def pair(script, rng, start_x=0, start_y=0, tail=0, seed=None):
    """The two strings of a script: a list of (kind, n) -- 'm' n columns with x == y, 'x' n with x != y, 'i' n query residues against
    blanks, 'd' n target residues against blanks, 'p' n columns blank in both.  seed: the (x, y) of a seed column behind them, or None
    for strings that end with the last counted column.  Returns a dict with the strings, both sequences (start_x / start_y residues
    in front, `tail` behind) and the summary's words."""
    qs, ts = [], []
    for kind, n in script:
        for _ in range(n):
            a = int(rng.integers(0, 20))
            b = a if kind == "m" else (a + 1 + int(rng.integers(0, 19))) % 20
            qs.append(BLANK if kind in "dp" else a)
            ts.append(BLANK if kind in "ip" else b)
    n = len(qs)
    q_seq = [int(x) for x in rng.integers(0, 20, size=start_x)] + [x for x in qs if x != BLANK] + [int(x) for x in rng.integers(0, 20, size=tail)]
    t_seq = [int(x) for x in rng.integers(0, 20, size=start_y)] + [x for x in ts if x != BLANK] + [int(x) for x in rng.integers(0, 20, size=tail)]
    if seed is not None:
        qs, ts = qs + [seed[0]], ts + [seed[1]]
    return dict(q=qs, t=ts, n=n, aln_len=n + 1, room=len(qs), start_x=start_x, start_y=start_y, N=len(q_seq), q_seq=q_seq, t_seq=t_seq, status=0,
                script=script)


def merged(script):
    """the script's runs as the rule sees them without EXTENDED: m and x are one op, equal neighbours are one run"""
    out = []
    for kind, n in script:
        op = {"m": R.M, "x": R.M, "i": R.I, "d": R.D, "p": R.P}[kind]
        if n:
            if out and out[-1][0] == op:
                out[-1][1] += n
            else:
                out.append([op, n])
    return [(n << 4) | op for op, n in out]


def cases():
    """name -> case.  Every shape twice: the strings end with column n - 1 (a look at column n is a read beyond the buffer), and a seed
    column stands behind them whose ops differ from the last run's (a look at it changes the words)."""
    rng = np.random.default_rng(2001)
    shapes = {}
    for n in ROUNDS:
        for kind in "mid":
            shapes["one %s run of %d" % (kind, n)] = dict(script=[(kind, n)])
    for e in (62, 63, 64, 65):
        shapes["a run ends at column %d" % e] = dict(script=[("m", e - 2), ("i", 3), ("m", 10)])
        shapes["the last run ends at column %d" % e] = dict(script=[("m", e - 1), ("d", 2)])
    for length in (64, 65, 128, 129):
        for a in (1, 30, 63, 64, 127):
            shapes["a run of %d from column %d" % (length, a)] = dict(script=[("m", a), ("d", length), ("x", 5)])
    shapes["= and X alternate"] = dict(script=[("m", 1), ("x", 1)] * 100)
    shapes["I directly followed by D"] = dict(script=[("m", 5), ("i", 3), ("d", 4), ("m", 5), ("d", 70), ("i", 70), ("x", 2)])
    shapes["P inside and at the ends"] = dict(script=[("p", 2), ("m", 5), ("p", 3), ("m", 2), ("i", 1), ("p", 66), ("d", 1), ("p", 1)])
    shapes["clipped at both ends"] = dict(script=[("m", 70), ("i", 2), ("m", 3)], start_x=7, start_y=3, tail=5)
    shapes["clipped in front only"] = dict(script=[("x", 4), ("d", 2), ("m", 3)], start_x=300, start_y=0, tail=0)
    shapes["no columns at all, clipped"] = dict(script=[], start_x=4, start_y=9, tail=6)
    out = {}
    for name, kw in shapes.items():
        out[name] = pair(rng=rng, **kw)
        last = kw["script"][-1][0] if kw["script"] else "m"
        out[name + ", a seed column behind"] = pair(rng=rng, seed=(BLANK, 3) if last in "mxi" else (3, 3), **kw)
    return out


def line_of(c, flags, N=None, status=0):
    words = [BLANK, flags, status, c["start_x"], c["start_y"], c["N"] if N is None else N, c["aln_len"], c["room"]] + c["q"] + c["t"]
    return " ".join(str(w) for w in words)


def want_of(c, flags, N=None, status=0):
    return R.encode(c["q"], c["t"], c["aln_len"], status, c["start_x"], c["start_y"], c["N"] if N is None else N, BLANK, flags)


def check_cases(drv):
    all_cases = cases()
    lines, wants, names = [], [], []
    for name, c in all_cases.items():
        for flags in ALL_FLAGS:
            rec, words, pads, over = want_of(c, flags)
            # the round trip, from the reference alone
            qs, ts = R.decode(words, c["q_seq"], c["t_seq"], c["start_x"], c["start_y"], BLANK)
            assert qs == c["q"][:c["n"]] and ts == c["t"][:c["n"]], name
            assert R.consumed(words) == (rec[2] - rec[1], rec[4] - rec[3]), name
            assert rec[0] == len(words) and over == 0 and rec[1:5] == (c["start_x"], rec[2], c["start_y"], rec[4])
            assert rec[6] == c["n"] - pads and all(0 < (w >> 4) for w in words)
            if not flags & R.CLIPS:
                assert all(w & 15 != R.S for w in words)
                assert all(a & 15 != b & 15 for a, b in zip(words, words[1:])), "neighbouring runs differ"
            if not flags & R.EXTENDED:
                runs = [w for w in words if w & 15 != R.S]
                assert runs == merged(c["script"]), name
            # the host helpers of the package are the same rule
            g_rec, g_words, g_pads, g_over = cigar.encode(c["q"], c["t"], BLANK, flags, c["start_x"], c["start_y"], c["N"], 0, skip_seed=c["room"] > c["n"])
            assert tuple(int(g_rec[k]) for k in R.RECORD_KEYS) == rec and g_words.tolist() == words and (g_pads, g_over) == (pads, over), name
            d_q, d_t = cigar.decode(g_words, c["q_seq"], c["t_seq"], c["start_x"], c["start_y"], BLANK)
            assert d_q.tolist() == qs and d_t.tolist() == ts
            lines.append(line_of(c, flags))
            wants.append((rec, words, pads, over))
            names.append((name, flags))
    # what the names promise, from the reference
    by = {k: v for k, v in zip(names, wants)}
    for n in ROUNDS:
        assert by[("one m run of %d" % n, 0)][1] == ([(n << 4) | R.M] if n else [])
        assert by[("one i run of %d, a seed column behind" % n, R.EXTENDED)][1] == ([(n << 4) | R.I] if n else [])
    rec, words, _p, _o = by[("= and X alternate", R.EXTENDED)]
    assert rec[0] == 200 == len(words) and [w & 15 for w in words[:2]] == [R.EQ, R.X] and by[("= and X alternate", 0)][1] == [(200 << 4) | R.M]
    assert [w & 15 for w in by[("I directly followed by D", 0)][1]] == [R.M, R.I, R.D, R.M, R.D, R.I, R.M]
    rec, words, pads, _o = by[("P inside and at the ends", 0)]
    assert pads == 72 and words[0] == (2 << 4) | R.P and words[-1] == (1 << 4) | R.P and (66 << 4) | R.P in words and rec[6] == 9
    assert by[("one m run of 65", R.CLIPS)][1] == [(65 << 4) | R.M], "start_x == 0 and q_end == N: no clip words"
    assert by[("clipped at both ends", R.CLIPS)][1] == [(7 << 4) | R.S, (70 << 4) | R.M, (2 << 4) | R.I, (3 << 4) | R.M, (5 << 4) | R.S]
    assert by[("clipped in front only", R.CLIPS | R.EXTENDED)][1] == [(300 << 4) | R.S, (4 << 4) | R.X, (2 << 4) | R.D, (3 << 4) | R.EQ]
    assert by[("no columns at all, clipped", R.CLIPS)][1] == [(4 << 4) | R.S, (6 << 4) | R.S] and by[("no columns at all, clipped", 0)][0][0] == 0
    for length in (64, 65, 128, 129):
        for a in (1, 30, 63, 64, 127):
            assert by[("a run of %d from column %d" % (length, a), R.EXTENDED)][1] == [(a << 4) | R.EQ, (length << 4) | R.D, (5 << 4) | R.X]
    # a query shorter than the strings say: no trailing clip and one overflow; a status that is not OK: an empty record
    c = all_cases["clipped at both ends"]
    for flags in ALL_FLAGS:
        lines.append(line_of(c, flags, N=c["N"] - 6))
        wants.append(want_of(c, flags, N=c["N"] - 6))
        assert wants[-1][3] == (1 if flags & R.CLIPS else 0) and wants[-1][1][-1] & 15 in (R.M, R.EQ)
        lines.append(line_of(c, flags, status=4))
        wants.append(want_of(c, flags, status=4))
        assert wants[-1] == ((0, 0, 0, 0, 0, 0, 0, 4), [], 0, 0)
        assert int(cigar.encode(c["q"], c["t"], BLANK, flags, 7, 3, c["N"], status=4)[0]["status"]) == 4
        assert cigar.encode(c["q"], c["t"], BLANK, flags, 7, 3, c["N"] - 6, skip_seed=False)[3] == wants[-2][3]
    # the ends are 64-bit sums saturated to 32 bits
    c = dict(all_cases["one m run of 65"], start_x=0xFFFFFFF0, start_y=0xFFFFFFFF)
    lines.append(line_of(c, 0))
    wants.append(want_of(c, 0))
    assert wants[-1][0][1:5] == (0xFFFFFFF0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    out = run(drv, "hits", lines)
    assert len(out) == len(lines)
    for line, (rec, words, pads, over) in zip(out, wants):
        got = [int(x) for x in line.split()]
        assert tuple(got[:8]) == rec and got[8:11] == [pads, over, len(words)] and got[11:] == words, line[:200]


def check_offsets(drv):
    big = R.MAX_RUN + 2                               # the most words one hit of a supported set can have
    sets = [[], [0], [5], [3, 0, 7, 0, 0, 11], [big] * 40, [1, big, 0, big] * 9]
    out = run(drv, "offsets", ["%d %s" % (len(s), " ".join(str(v) for v in s)) for s in sets])
    for s, line in zip(sets, out):
        got = [int(x) for x in line.split()]
        want = R.offsets([(v,) for v in s])
        assert got[0] == want[-1] == sum(s) and got[1:] == want
    assert sum(sets[4]) > 2 ** 32 and sum(sets[5]) > 2 ** 32
    limits = [(0, 0), (2 ** 27 - 2, 3), (2 ** 27 - 1, 4), (2 ** 27, 1), (256, 2), (257, 8), (2 ** 32 - 1, 0x80000000)]
    out = run(drv, "limits", ["%d %d" % l for l in limits])
    for (max_len, flags), line in zip(limits, out):
        assert [int(x) for x in line.split()] == [int(2 * max_len + 2 < 2 ** 28), int(flags in ALL_FLAGS), (max_len + 255) // 256]


def test_constructed_pairs(driver):
    check_cases(driver)


def test_offsets_and_limits(driver):
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


def test_cigars_views_and_text():
    rec = np.zeros(3, dtype=cigar.RECORD_DTYPE)
    rec[0] = (3, 2, 62, 5, 64, 50, 62, 0)
    rec[1] = (0, 0, 0, 0, 0, 0, 0, 4)
    rec[2] = (4, 1, 9, 0, 7, 6, 9, 0)
    words = np.array([(57 << 4) | R.M, (2 << 4) | R.D, (3 << 4) | R.M, (1 << 4) | R.S, (6 << 4) | R.EQ, (1 << 4) | R.X, (1 << 4) | R.I], dtype=np.uint32)
    got = cigar.Cigars(np.array([4, 0, 9], dtype=np.uint32), rec, {}, np.array([0, 3, 3, 7], dtype=np.uint64), words)
    assert len(got) == 3 and got.ops(0).tolist() == words[:3].tolist() and got.ops(1).tolist() == [] and got.ops(2).dtype == np.uint32
    assert got.text(0) == "57M2D3M" and got.text(1) == "" and got.text(2) == "1S6=1X1I" == R.text(words[3:].tolist())
    assert got.paf(0, "q one", 70, "t1", 80, 123.5) == "q one\t70\t2\t62\t+\tt1\t80\t5\t64\t50\t62\t255\taf:f:123.5\tcg:Z:57M2D3M"
    assert cigar.text_of([(0x0FFFFFFF << 4) | R.P]) == "268435455P"
    with pytest.raises(ValueError):
        cigar.encode([1], [1], BLANK, 4)
    with pytest.raises(ValueError):
        cigar.decode([(5 << 4) | R.M], [1, 2], [1, 2, 3, 4, 5], 0, 0, BLANK)
    assert cigar.CIGAR_RECORD_DTYPE is cigar.RECORD_DTYPE


# ---------------------------------------------------------------- the companion header and its mirrors
def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared(path):
    return sorted(set(re.findall(r"\b(aln_[a-z_0-9]+)\s*\(", strip_comments(open(path).read()))))


def test_the_companion_header_declares_the_cigar_exports():
    assert _ffi.CIGAR_EXPORTS == ["aln_seqset_held_cigar_fill", "aln_seqset_held_cigar_plan"]
    assert declared(os.path.join(ROOT, "include", "aligner_hip_cigar.h")) == sorted(_ffi.CIGAR_EXPORTS)
    assert len(declared(os.path.join(ROOT, "include", "aligner_hip.h"))) == 61         # the main header is as it was
    for other in (_ffi.EXPORTS, _ffi.CLUSTER_EXPORTS, _ffi.PREFILTER_EXPORTS, _ffi.SEARCH_EXPORTS, _ffi.PROFILE_EXPORTS, _ffi.MSA_EXPORTS):
        assert not set(_ffi.CIGAR_EXPORTS) & set(other)
    assert "aln_cigar.hip" in native_build.SOURCES and "aln_cigar_rules.h" in native_build.HEADERS
    assert any(h.endswith("aligner_hip_cigar.h") for h in native_build.HEADERS)
    assert (_ffi.CIGAR_EXTENDED, _ffi.CIGAR_CLIPS) == (R.EXTENDED, R.CLIPS) == (cigar.EXTENDED, cigar.CLIPS)
    header = strip_comments(open(os.path.join(ROOT, "include", "aligner_hip_cigar.h")).read())
    ops = dict(re.findall(r"#define ALN_CIGAR_(M|I|D|S|P|EQ|X) (\d+)u", header))
    assert {k: int(v) for k, v in ops.items()} == dict(M=R.M, I=R.I, D=R.D, S=R.S, P=R.P, EQ=R.EQ, X=R.X)


def test_the_library_exports_them_with_argtypes():
    native_build.build()
    lib = _ffi.load()
    for sym in _ffi.CIGAR_EXPORTS:
        fn = getattr(lib, sym)
        assert fn.argtypes is not None and fn.restype is C.c_int, sym
    assert lib.aln_abi_version() == 2


def test_every_export_is_called_from_c99():
    src = strip_comments(open(os.path.join(ROOT, "tests", "abi_cigar.c")).read())
    for sym in _ffi.CIGAR_EXPORTS:
        assert re.search(r"\b%s\s*\(" % sym, src), sym


def test_the_header_compiles_as_c99_and_the_layouts_match(tmp_path):
    native_build.build()
    src = str(tmp_path / "only.c")
    with open(src, "w") as fh:
        fh.write('#include "aligner_hip_cigar.h"\nint main(void) { return (int)sizeof(aln_cigar_record) - 32; }\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                           str(tmp_path / "only.o")])
    exe = native_build.build_cigar_harness()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("layout ")]
    assert [l[1] for l in lines] == ["aln_cigar_record", "aln_cigar_summary"]
    for l, cls in zip(lines, (_ffi.CigarRecord, _ffi.CigarSummary)):
        assert int(l[2]) == C.sizeof(cls)
        fields = [(l[k], int(l[k + 1]), int(l[k + 2])) for k in range(3, len(l), 3)]
        assert fields == [(name, getattr(cls, name).offset, getattr(cls, name).size) for name, _t in cls._fields_]
    assert C.sizeof(_ffi.CigarRecord) == 32 and C.sizeof(_ffi.CigarSummary) == 48
    assert [(n, _ffi.CigarRecord.__dict__[n].offset) for n, _t in _ffi.CigarRecord._fields_] == [
        ("n_ops", 0), ("q_start", 4), ("q_end", 8), ("t_start", 12), ("t_end", 16), ("matches", 20), ("block", 24), ("status", 28)]
    assert [(n, _ffi.CigarSummary.__dict__[n].offset) for n, _t in _ffi.CigarSummary._fields_] == [
        ("held", 0), ("listed", 8), ("total_ops", 16), ("failed", 24), ("padded", 28), ("overflow", 32), ("reserved", 36)]
    assert cigar.RECORD_DTYPE.itemsize == 32 and list(cigar.RECORD_DTYPE.names) == [f[0] for f in _ffi.CigarRecord._fields_] == list(R.RECORD_KEYS)
    assert [cigar.RECORD_DTYPE.fields[n][1] for n in cigar.RECORD_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert cigar.RECORD_DTYPE["status"] == np.dtype("<i4")
    assert list(cigar.SUMMARY_KEYS) == [f[0] for f in _ffi.CigarSummary._fields_][:-1] == list(R.SUMMARY_KEYS)


# ---------------------------------------------------------------- refusals that need no device, and the command's argument errors
def test_refusals_without_a_device():
    native_build.build()
    lib = _ffi.load()
    INV = _ffi.ERR_INVALID_ARGUMENT
    rec = (_ffi.CigarRecord * 2)(_ffi.CigarRecord(7, 7, 7, 7, 7, 7, 7, 7), _ffi.CigarRecord(7, 7, 7, 7, 7, 7, 7, 7))
    which = (C.c_uint32 * 2)(0, 1)
    summ = _ffi.CigarSummary(9, 9, 9, 9, 9, 9, (C.c_uint32 * 3)(9, 9, 9))
    ops = (C.c_uint32 * 4)(7, 7, 7, 7)
    off = (C.c_uint64 * 3)(7, 7, 7)
    # a null set
    assert lib.aln_seqset_held_cigar_plan(None, 0, which, 2, rec, C.byref(summ)) == INV and b"null" in lib.aln_last_error()
    assert lib.aln_seqset_held_cigar_plan(None, 3, None, 0, None, C.byref(summ)) == INV and b"null" in lib.aln_last_error()
    # any bit but the two
    for flags in (4, 8, 7, 0x80000000, 0x80000001):
        assert lib.aln_seqset_held_cigar_plan(None, flags, which, 2, rec, C.byref(summ)) == INV and b"flag" in lib.aln_last_error()
    # null which, records, summary; a list too long
    assert lib.aln_seqset_held_cigar_plan(None, 0, None, 2, rec, C.byref(summ)) == INV and b"null" in lib.aln_last_error()
    assert lib.aln_seqset_held_cigar_plan(None, 0, which, 2, None, C.byref(summ)) == INV and b"null" in lib.aln_last_error()
    assert lib.aln_seqset_held_cigar_plan(None, 0, which, 2, rec, None) == INV and b"null" in lib.aln_last_error()
    assert lib.aln_seqset_held_cigar_plan(None, 0, which, 0x7FFFFFF1, rec, C.byref(summ)) == INV and b"too long" in lib.aln_last_error()
    # a fill without a plan (without a set there is none)
    assert lib.aln_seqset_held_cigar_fill(None, ops, 4, off, 3) == INV
    assert lib.aln_seqset_held_cigar_fill(None, None, 0, None, 0) == INV
    assert all(tuple(getattr(r, f[0]) for f in _ffi.CigarRecord._fields_) == (7,) * 8 for r in rec) and list(ops) == [7] * 4 and list(off) == [7] * 3
    assert [getattr(summ, f[0]) for f in _ffi.CigarSummary._fields_[:-1]] == [9] * 6 and list(summ.reserved) == [9] * 3


def test_the_commands_argument_errors(capsys):
    path = os.path.join(ROOT, "tests", "golden", "protein.fasta")
    for bad, word in ((["--paf", "x.paf"], "held hits"), (["--eqx"], "--paf"), (["--f-min", "30", "--eqx"], "--paf"), (["--f-min", "30", "--paf"], "--paf"),
                      (["--kmer", "3", "--paf", "x.paf"], "held hits"), (["--f-min", "30", "--cluster", "greedy", "--paf", "x.paf"], "--cluster"),
                      (["--best", "3", "--cluster", "components", "--paf", "x.paf", "--eqx"], "--cluster"),
                      (["--heuristic", "--kd", "1", "--r-squared", "0.9", "--paf", "x.paf"], "--heuristic")):
        with pytest.raises(SystemExit) as e:
            allpairs.main(["-i", path] + bad)
        assert e.value.code == 2
        assert word in capsys.readouterr().err, bad
    assert not os.path.exists("x.paf")
