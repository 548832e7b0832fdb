"""The LDS carve-up of the fast batch kernels (aln_fast_lds_bytes, aln_device.h -- the one place host and kernel take it from)
and the routing rule that admits an alphabet to them (ALN_FAST_LDS, aln_scheme_rules.h), compiled for the host; no GPU.  The
C5 workgroup (24 x 24, R = 8 profiles, four waves' feed rings) takes 53 312 bytes: within the 53 760 that let three workgroups
share a CU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include <cmath>
#define __host__
#define __device__
struct uint4;
#include "aln_device.h"
#include "aln_scheme_rules.h"
int main()
{
    // the C5 workgroup: 24 x 24, four profiles of 24 x 64 x ALN_FULL_R bytes, four waves' feed rings
    const unsigned prof = 24u * 64u * ALN_FULL_R;
    printf("c5 %u rings_at %u\n", aln_fast_lds_bytes(24, 24, prof, ALN_FEED_BYTES), aln_fast_lds_bytes(24, 24, prof, 0));
    const unsigned letters[4] = {4, 20, 24, 30};
    for (unsigned a : letters) {
        const double one = 1.0;
        AlnScheme s = aln_scheme_scan(true, 2.0, 1.0, &one, 1);
        aln_scheme_route(s, false, a, a, 1000, false, false, false, false, ALN_FULL_R);
        printf("%u %d %llu %u\n", a, s.fast ? 1 : 0, (unsigned long long)s.fast_lds, aln_fast_lds_bytes(a, a, a * 64u * ALN_FULL_R, ALN_FEED_BYTES));
    }
    AlnScheme s = aln_scheme_scan(true, 2.0, 1.0, nullptr, 0);
    aln_scheme_route(s, false, 31, 31, 1000, false, false, false, false, ALN_FULL_R);
    printf("31 %d\n", s.fast ? 1 : 0);
    return 0;
}
"""


def test_lds_carve_up_keeps_three_workgroups_per_cu(tmp_path):
    """aln_fast_lds_bytes is the one carve-up host and kernel share: the C5 workgroup stays within 53 760 bytes (three per CU), and
    ALN_FAST_LDS admits alphabets of 4, 20, 24 and 30 letters, not 31."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.fail("no C++ compiler (%s) to build the carve-up driver" % cxx)
    src, exe = tmp_path / "lds.cpp", tmp_path / "lds"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "aligner_amd", "csrc"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    c5 = lines[0].split()
    assert int(c5[1]) <= 53760 and int(c5[1]) == 53312
    assert int(c5[1]) - int(c5[3]) == 4 * (192 + 272)         # per wave: query ring, boundary ring (ints 0 .. 64 and padding)
    for line, a in zip(lines[1:5], (4, 20, 24, 30)):
        f = line.split()
        assert int(f[0]) == a and f[1] == "1", line
        assert int(f[2]) == ((a * a * 4 + 15) & ~15) + 4 * a * 64 * 8 <= 65536, line
        assert int(f[3]) == int(f[2]) + 4 * (192 + 272), line
    assert lines[5].split() == ["31", "0"]
