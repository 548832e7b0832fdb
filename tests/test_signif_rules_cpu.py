"""The rule of aln_seqset_held_significance (aln_signif_rules.h; no GPU): the header compiled into a driver with the host compiler and
checked against the numpy restatement in signif_ref.py -- integer-valued scores, scores of a wide dynamic range for which the
rule's order shows in the bits, failed copies at the accumulator edges, no copy left -- plus the record's layout (also from C99),
the export and its argument types, the refusal that needs no device, the formulas of the Python layer and the refusals of
`allpairs --shuffles`."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import signif_ref  # noqa: E402
from aligner_amd import _ffi  # noqa: E402
from aligner_amd import allpairs  # noqa: E402
from aligner_amd import seqset as seqset_module  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_PAIR = [1, 2, 63, 64, 65, 127, 128, 129, 4999]

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstddef>
#include <vector>
#include "aln_signif_rules.h"
typedef unsigned long long ull;
static ull bits(double v) { uint64_t b; memcpy(&b, &v, 8); return (ull)b; }
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "layout")) {
        printf("%u %u %u %u %u %u %u %u %u\n", (unsigned)sizeof(aln_signif_record), (unsigned)offsetof(aln_signif_record, sum),
               (unsigned)offsetof(aln_signif_record, sum_sq), (unsigned)offsetof(aln_signif_record, f_max), (unsigned)offsetof(aln_signif_record, n_ok),
               (unsigned)offsetof(aln_signif_record, n_ge), (unsigned)offsetof(aln_signif_record, status), (unsigned)offsetof(aln_signif_record, first_bad),
               (unsigned)offsetof(aln_signif_record, reserved));
        const aln_signif_record e = aln_signif_empty();
        printf("%llx %llx %llx %u %u %d %u %llu\n", bits(e.sum), bits(e.sum_sq), bits(e.f_max), e.n_ok, e.n_ge, e.status, e.first_bad, (ull)e.reserved);
        return 0;
    }
    if (!strcmp(argv[1], "reduce")) {           // stdin: <per_pair> <f_hit bits>, then per copy <status> <f bits>; repeated
        ull per, hb;
        while (scanf("%llu %llx", &per, &hb) == 2) {
            std::vector<double> f(per);
            std::vector<int32_t> st(per);
            for (ull s = 0; s < per; ++s) {
                int v; ull b;
                if (scanf("%d %llx", &v, &b) != 2) return 4;
                st[s] = v; uint64_t x = b; memcpy(&f[s], &x, 8);
            }
            double hit; { uint64_t x = hb; memcpy(&hit, &x, 8); }
            // once from plain arrays, once from summaries (the strides the kernel reads with)
            const aln_signif_record a = aln_signif_reduce(f.data(), 8, st.data(), 4, (uint32_t)per, hit);
            std::vector<aln_pair_result> res(per);
            memset(res.data(), 0x5a, per * sizeof(aln_pair_result));
            for (ull s = 0; s < per; ++s) { res[s].f = f[s]; res[s].status = st[s]; }
            const aln_signif_record b = aln_signif_reduce(&res[0].f, sizeof(aln_pair_result), &res[0].status, sizeof(aln_pair_result), (uint32_t)per, hit);
            if (memcmp(&a, &b, sizeof a)) return 5;
            printf("%llx %llx %llx %u %u %d %u %llu\n", bits(a.sum), bits(a.sum_sq), bits(a.f_max), a.n_ok, a.n_ge, a.status, a.first_bad, (ull)a.reserved);
        }
        return 0;
    }
    return 2;
}
"""

C99 = r"""
#include <stddef.h>
#include "aligner_hip.h"
#define PIN(name, cond) typedef char pin_##name[(cond) ? 1 : -1]
PIN(size, sizeof(aln_signif_record) == 48);
PIN(sum, offsetof(aln_signif_record, sum) == 0);
PIN(sum_sq, offsetof(aln_signif_record, sum_sq) == 8);
PIN(f_max, offsetof(aln_signif_record, f_max) == 16);
PIN(n_ok, offsetof(aln_signif_record, n_ok) == 24);
PIN(n_ge, offsetof(aln_signif_record, n_ge) == 28);
PIN(status, offsetof(aln_signif_record, status) == 32);
PIN(first_bad, offsetof(aln_signif_record, first_bad) == 36);
PIN(reserved, offsetof(aln_signif_record, reserved) == 40);
int (*const held_significance)(aln_seqset *, const aln_params *, const aln_shuffle_spec *, const uint32_t *, uint64_t, aln_signif_record *, double *,
                               uint32_t *) = aln_seqset_held_significance;
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.fail("no C++ compiler (%s) to build the significance-rule driver" % cxx)
    tmp = tmp_path_factory.mktemp("signif_rules")
    src = os.path.join(str(tmp), "drv.cpp")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(str(tmp), "drv")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "aligner_amd", "csrc"), src,
                           "-o", exe])
    return exe


def bits(f):
    return struct.unpack("<Q", struct.pack("<d", float(f)))[0]


def run_cases(drv, cases):
    """cases: (f, status, f_hit) -> records as signif_ref.RECORD"""
    text = []
    for f, status, f_hit in cases:
        text.append("%d %x" % (len(f), bits(f_hit)))
        text.append(" ".join("%d %x" % (int(s), bits(v)) for s, v in zip(status, f)))
    out = subprocess.run([drv, "reduce"], check=True, capture_output=True, text=True, input="\n".join(text) + "\n").stdout.splitlines()
    assert len(out) == len(cases)
    rec = np.zeros(len(cases), dtype=signif_ref.RECORD)
    for i, line in enumerate(out):
        t = line.split()
        rec[i] = (struct.unpack("<d", struct.pack("<Q", int(t[0], 16)))[0], struct.unpack("<d", struct.pack("<Q", int(t[1], 16)))[0],
                  struct.unpack("<d", struct.pack("<Q", int(t[2], 16)))[0], int(t[3]), int(t[4]), int(t[5]), int(t[6]), int(t[7]))
    return rec


def check(drv, cases):
    got = run_cases(drv, cases)
    for i, (f, status, f_hit) in enumerate(cases):
        want = signif_ref.reduce_one(f, status, f_hit)
        assert got[i].tobytes() == want.tobytes(), (len(f), got[i], want)
    return got


def wide(rng, n):
    """1e-3 .. 1e9 in magnitude, mixed in sign: sums whose bits depend on the order of the additions"""
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 9, n)


def test_record_layout_and_empty_accumulator(driver, tmp_path):
    out = subprocess.run([driver, "layout"], check=True, capture_output=True, text=True).stdout.splitlines()
    assert [int(v) for v in out[0].split()] == [48, 0, 8, 16, 24, 28, 32, 36, 40]
    assert out[1].split() == ["0", "0", "%x" % bits(float("-inf")), "0", "0", "0", str(0xFFFFFFFF), "0"]
    assert C.sizeof(_ffi.SignifRecord) == seqset_module.SIGNIF_RECORD_DTYPE.itemsize == signif_ref.RECORD.itemsize == 48
    names = [n for n, _ in _ffi.SignifRecord._fields_]
    assert names == list(seqset_module.SIGNIF_RECORD_DTYPE.names) == list(signif_ref.RECORD.names)
    assert [getattr(_ffi.SignifRecord, n).offset for n in names] == [seqset_module.SIGNIF_RECORD_DTYPE.fields[n][1] for n in names] == [0, 8, 16, 24, 28, 32, 36, 40]
    # the public header alone, as C99: the same pins, and the export's type
    cc = os.environ.get("CC", "gcc")
    src = str(tmp_path / "pin.c")
    with open(src, "w") as fh:
        fh.write(C99)
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "pin.o")])


@pytest.mark.parametrize("per_pair", PER_PAIR)
def test_integer_valued_scores(driver, per_pair):
    rng = np.random.default_rng(per_pair)
    cases = []
    for f_hit in (0.0, 37.0, -5.0, 1e9):
        f = rng.integers(-40, 120, per_pair).astype(np.float64)
        cases.append((f, np.zeros(per_pair, dtype=np.int32), f_hit))
    got = check(driver, cases)
    for (f, _, f_hit), r in zip(cases, got):             # integers: any order gives these
        assert r["sum"] == f.sum() and r["sum_sq"] == (f * f).sum() and r["f_max"] == f.max()
        assert r["n_ok"] == per_pair and r["n_ge"] == int((f >= f_hit).sum()) and r["status"] == 0 and r["first_bad"] == 0xFFFFFFFF


@pytest.mark.parametrize("per_pair", PER_PAIR)
def test_wide_range_scores_follow_the_rules_order(driver, per_pair):
    rng = np.random.default_rng(1000 + per_pair)
    cases = [(wide(rng, per_pair), np.zeros(per_pair, dtype=np.int32), 10.0 ** e) for e in (-4, 0, 3, 6, 10)]
    got = check(driver, cases)
    if per_pair >= 63:
        # the input tells the rule's order from one ascending sum (with one or two copies there is only one order)
        differs = [bits(r["sum"]) != bits(signif_ref.sequential(f, st)[0]) or bits(r["sum_sq"]) != bits(signif_ref.sequential(f, st)[1])
                   for (f, st, _), r in zip(cases, got)]
        assert any(differs), per_pair
    for (f, _, f_hit), r in zip(cases, got):
        assert r["f_max"] == f.max() and r["n_ge"] == int((f >= f_hit).sum())


@pytest.mark.parametrize("per_pair", PER_PAIR)
def test_failed_copies(driver, per_pair):
    """Failed copies at 0, 63, 64 and the last copy (where the hit has them), one at a time and together; negative scores only (a
    maximum that started at 0 would show); every copy failed."""
    rng = np.random.default_rng(2000 + per_pair)
    spots = sorted({p for p in (0, 63, 64, per_pair - 1) if p < per_pair})
    cases = []
    for group in [[p] for p in spots] + [spots]:
        f = wide(rng, per_pair)
        st = np.zeros(per_pair, dtype=np.int32)
        for j, p in enumerate(group):
            st[p] = (_ffi.ERR_EMPTY_SEQUENCE, _ffi.ERR_NO_POSITIVE_CELL)[j % 2]
            f[p] = 0.0 if j % 2 else 1e12                 # what a failed copy's summary holds must not count
        cases.append((f, st, 1.0))
    neg = -np.abs(wide(rng, per_pair)) - 1.0
    cases.append((neg, np.zeros(per_pair, dtype=np.int32), -3.0))
    dead = np.full(per_pair, _ffi.ERR_EMPTY_SEQUENCE, dtype=np.int32)
    dead[0] = _ffi.ERR_NO_POSITIVE_CELL
    cases.append((wide(rng, per_pair), dead, 0.0))
    got = check(driver, cases)
    for (f, st, f_hit), r in zip(cases[:-2], got[:-2]):
        bad = np.flatnonzero(st)
        assert r["n_ok"] == per_pair - len(bad) and r["first_bad"] == bad[0] and r["status"] == st[bad[0]]
        ok = st == 0
        assert r["n_ge"] == int((f[ok] >= f_hit).sum())
        assert r["f_max"] == (f[ok].max() if ok.any() else float("-inf"))
    assert got[-2]["f_max"] == neg.max() < 0 and got[-2]["n_ok"] == per_pair
    last = got[-1]
    assert last["n_ok"] == 0 and last["n_ge"] == 0 and last["f_max"] == float("-inf") and last["first_bad"] == 0
    assert last["status"] == _ffi.ERR_NO_POSITIVE_CELL and bits(last["sum"]) == 0 and bits(last["sum_sq"]) == 0


# ---------------------------------------------------------------- the library and the Python layer
@pytest.fixture(scope="module")
def lib():
    from aligner_amd import build as native_build
    native_build.build()
    return _ffi.load()


def test_library_exports_significance_with_the_headers_arguments(lib):
    text = open(os.path.join(ROOT, "include", "aligner_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "aln_seqset_held_significance" in _ffi.EXPORTS and hasattr(lib, "aln_seqset_held_significance")
    decl = re.search(r"\baln_seqset_held_significance\s*\(([^;]*)\)\s*;", hdr)
    assert decl
    args = [" ".join(a.split()) for a in decl.group(1).split(",") if a.strip()]
    assert args == ["aln_seqset *set", "const aln_params *params", "const aln_shuffle_spec *spec", "const uint32_t *keep", "uint64_t n_keep",
                    "aln_signif_record *records", "double *f", "uint32_t *lengths"]
    at = lib.aln_seqset_held_significance.argtypes
    assert len(at) == len(args) == 8
    assert at[1] == C.POINTER(_ffi.Params) and at[2] == C.POINTER(_ffi.ShuffleSpec) and at[4] is C.c_uint64
    assert all(at[i] is C.c_void_p for i in (0, 3, 5, 6, 7))
    body = hdr[hdr.index("typedef struct aln_signif_record {"):hdr.index("} aln_signif_record;")]
    assert re.findall(r"(\w+)\s*;", body) == list(signif_ref.RECORD.names)
    assert lib.aln_abi_version() == 2
    rust = open(os.path.join(ROOT, "rust", "aligner-core-hip", "src", "lib.rs")).read()
    assert "pub fn aln_seqset_held_significance(" in rust and "pub struct AlnSignifRecord" in rust
    assert "aln_seqset_held_significance" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_null_handle_is_refused_and_writes_nothing(lib):
    rec = np.full(2, 7, dtype=np.uint8).repeat(48).view(seqset_module.SIGNIF_RECORD_DTYPE)
    before = rec.tobytes()
    keep = np.array([0, 1], dtype=np.uint32)
    spec = _ffi.ShuffleSpec(1, 0, 10, 6)
    p = _ffi.Params()
    assert lib.aln_seqset_held_significance(None, C.byref(p), C.byref(spec), keep.ctypes.data, 2, rec.ctypes.data, None, None) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_seqset_held_significance(None, None, None, None, 0, None, None, None) == _ffi.ERR_INVALID_ARGUMENT
    assert rec.tobytes() == before
    assert callable(seqset_module.HeldHits.significance) and callable(seqset_module.HeldHits.p_values)


def test_formulas_of_the_python_layer():
    rec = np.zeros(5, dtype=seqset_module.SIGNIF_RECORD_DTYPE)
    # 4 copies 1, 2, 3, 6: mean 3, population variance (1 + 4 + 9 + 36) / 4 - 9 = 3.5
    rec[0] = (12.0, 50.0, 6.0, 4, 1, 0, 0xFFFFFFFF, 0)
    # every copy 5.0: sd = 0
    rec[1] = (15.0, 75.0, 5.0, 3, 3, 0, 0xFFFFFFFF, 0)
    # no copy left
    rec[2] = (0.0, 0.0, float("-inf"), 0, 0, _ffi.ERR_EMPTY_SEQUENCE, 0, 0)
    # rounding puts sum_sq / n below mean^2: clamped
    rec[3] = (3.0, float(np.nextafter(3.0, 0.0)), 1.0, 3, 0, 0, 0xFFFFFFFF, 0)
    # the hit equals the mean of identical copies: 0 / 0
    rec[4] = (15.0, 75.0, 5.0, 3, 3, _ffi.ERR_NO_POSITIVE_CELL, 2, 0)
    f_hit = np.array([6.0, 9.0, 4.0, 2.0, 5.0])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with np.errstate(all="raise"):
            s = seqset_module.significance_from_records(rec, f_hit)
    assert s.dtype == seqset_module.SIGNIF_DTYPE
    assert s["mean"][0] == 3.0 and s["sd"][0] == np.sqrt(3.5) and s["z"][0] == 3.0 / np.sqrt(3.5) and s["p_emp"][0] == 2.0 / 5.0
    assert s["mean"][1] == 5.0 and s["sd"][1] == 0.0 and s["z"][1] == float("inf") and s["p_emp"][1] == 1.0
    assert np.isnan(s["mean"][2]) and np.isnan(s["sd"][2]) and np.isnan(s["z"][2]) and s["p_emp"][2] == 1.0 and s["n_ok"][2] == 0
    assert s["status"][2] == _ffi.ERR_EMPTY_SEQUENCE
    assert s["sd"][3] == 0.0 and s["z"][3] == float("inf") and s["p_emp"][3] == 0.25
    assert s["sd"][4] == 0.0 and np.isnan(s["z"][4]) and s["status"][4] == _ffi.ERR_NO_POSITIVE_CELL
    assert s["n_ok"].tolist() == [4, 3, 0, 3, 3]
    assert len(seqset_module.significance_from_records(rec[:0], f_hit[:0])) == 0


def test_python_checks_per_pair_before_it_sizes_the_score_arrays():
    held = seqset_module.HeldHits.__new__(seqset_module.HeldHits)
    held.owner, held.count, held.semantics = None, 3, _ffi.CORE_LOCAL       # no set, no library: the check comes first
    for per_pair in (0, -1, (1 << 20) + 1):
        with pytest.raises(ValueError, match="per_pair"):
            held.significance_records(np.eye(4), 11, 2, 1, per_pair=per_pair, scores=True)


@pytest.mark.parametrize("argv", [
    ["--shuffles", "10"],                                             # no held pass
    ["--shuffles", "10", "--heuristic", "--kd", "1", "--r-squared", "1"],
    ["--shuffles", "10", "--best", "3", "--heuristic"],
    ["--shuffles", "0", "--best", "3"],
    ["--shuffles", str((1 << 20) + 1), "--f-min", "30"],
    ["--seed", "5", "--best", "3"],                                   # a seed without copies
])
def test_allpairs_refuses_before_anything_is_read(argv, capsys):
    with pytest.raises(SystemExit) as e:
        allpairs.main(["-i", os.path.join(ROOT, "no", "such.fasta")] + argv)
    assert e.value.code == 2
    assert "--shuffles" in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["--shuffles", "10", "--best", "3"], ["--shuffles", str(1 << 20), "--f-min", "30", "--seed", "9"]])
def test_allpairs_accepts_shuffles_with_a_held_pass(argv):
    """Accepted arguments get as far as the input file (which is not there); no device is asked for."""
    with pytest.raises(OSError):
        allpairs.main(["-i", os.path.join(ROOT, "no", "such.fasta")] + argv)
