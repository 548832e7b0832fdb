"""The arena layouts without a GPU: aligner_amd/csrc/aln_arena_rules.h driven through a small C++ program that prints where every piece
of every layout lands, compared with a model of the formula the host has always used: the running sum of align256(max(bytes, 4)) in
the order the pieces are taken.  The same driver is also built as a stand-alone program with -fsanitize=address,undefined and run
directly."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from aligner_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)
GREEDY, COMPONENTS = 1, 0
MISC_WORDS, CIGAR_MISC_WORDS, CIGAR_TILE = 8, 4, 256

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "aln_arena_rules.h"
// one line per case: the sizing pass's total, the placing pass's total, then every piece's offset in the order of the struct's
// fields below (-1: the layout has no such piece)
static std::vector<uint8_t> g_room;
static uint8_t *g_base;
static uint8_t *room_of(size_t bytes)
{
    g_room.assign(bytes + 256, 0);
    g_base = g_room.data() + ((256 - (uintptr_t)g_room.data() % 256) % 256);
    return g_base;
}
static void show(size_t sized, size_t placed, std::initializer_list<const void *> pieces)
{
    printf("%zu %zu", sized, placed);
    for (const void *p : pieces) printf(" %" PRId64, p ? (int64_t)((const uint8_t *)p - g_base) : (int64_t)-1);
    printf("\n");
}
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    uint64_t v[6];
    if (!strcmp(argv[1], "sizes")) {
        printf("%zu %zu %zu %zu %u %u %u %u\n", sizeof(aln_cluster_record), sizeof(aln_profile_record), sizeof(aln_msa_record), sizeof(aln_cigar_record),
               (unsigned)ALN_PROFILE_MISC_WORDS, (unsigned)ALN_MSA_MISC_WORDS, (unsigned)ALN_CIGAR_MISC_WORDS, (unsigned)ALN_CLUSTER_GREEDY);
        return 0;
    }
    if (!strcmp(argv[1], "cluster")) {         // `mode n m room tiles with_len`
        while (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, v, v + 1, v + 2, v + 3, v + 4, v + 5) == 6) {
            ClusterBufs b;
            const size_t sized = cluster_carve(nullptr, (uint32_t)v[0], v[1], v[2], v[3], v[4], v[5] != 0, &b);
            if (b.misc || b.label || b.rec) return 4;      // (a null base places nothing)
            const size_t placed = cluster_carve(room_of(sized), (uint32_t)v[0], v[1], v[2], v[3], v[4], v[5] != 0, &b);
            show(sized, placed, {b.misc, b.label, b.aux0, b.aux1, b.aux2, b.key, b.size, b.cedges, b.ea, b.eb, b.len, b.tile_off, b.tile_count, b.rec});
        }
        return 0;
    }
    if (!strcmp(argv[1], "profile")) {         // `n held n_centers total`
        while (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, v, v + 1, v + 2, v + 3) == 4) {
            ProfileBufs b;
            const size_t sized = profile_carve(nullptr, v[0], v[1], v[2], v[3], &b);
            if (b.misc || b.out) return 4;
            const size_t placed = profile_carve(room_of(sized), v[0], v[1], v[2], v[3], &b);
            show(sized, placed, {b.misc, b.hit_q, b.hit_t, b.label, b.slot_of, b.centers, b.off, b.rec, b.out});
        }
        return 0;
    }
    if (!strcmp(argv[1], "msa_plan")) {        // `n held n_centers n_ins`
        while (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, v, v + 1, v + 2, v + 3) == 4) {
            MsaPlanBufs b;
            const size_t sized = msa_plan_carve(nullptr, v[0], v[1], v[2], v[3], &b);
            if (b.misc || b.col) return 4;
            const size_t placed = msa_plan_carve(room_of(sized), v[0], v[1], v[2], v[3], &b);
            show(sized, placed, {b.misc, b.hit_q, b.hit_t, b.label, b.slot_of, b.centers, b.off, b.rec, b.mark, b.ins, b.col});
            // what the fill does: the same counts on the same base find the same tables
            MsaPlanBufs again;
            msa_plan_carve(g_base, v[0], v[1], v[2], v[3], &again);
            if (memcmp(&again, &b, sizeof b) != 0) return 5;
        }
        return 0;
    }
    if (!strcmp(argv[1], "msa_fill")) {        // `held n_centers bytes total_rows`
        while (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, v, v + 1, v + 2, v + 3) == 4) {
            MsaFillBufs b;
            const size_t sized = msa_fill_carve(nullptr, v[0], v[1], v[2], v[3], &b);
            if (b.byte_off || b.out) return 4;
            const size_t placed = msa_fill_carve(room_of(sized), v[0], v[1], v[2], v[3], &b);
            show(sized, placed, {b.byte_off, b.row_off, b.taken, b.list, b.hit_row, b.row_hit, b.out});
        }
        return 0;
    }
    if (!strcmp(argv[1], "cigar")) {           // `n`
        while (scanf("%" SCNu64, v) == 1) {
            CigarBufs b;
            const size_t sized = cigar_carve(nullptr, v[0], &b);
            if (b.misc || b.tile_off) return 4;
            const size_t placed = cigar_carve(room_of(sized), v[0], &b);
            show(sized, placed, {b.misc, b.list, b.rec, b.off, b.tile_sum, b.tile_off});
            CigarBufs again;
            cigar_carve(g_base, v[0], &again);
            if (memcmp(&again, &b, sizeof b) != 0) return 5;
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
    return build_driver(tmp_path_factory.mktemp("arena_rules"))


def run(drv, what, lines):
    out = subprocess.run([drv, what], capture_output=True, text=True, input="\n".join(lines) + "\n", timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return [[int(v) for v in line.split()] for line in out.stdout.splitlines()]


# ---------------------------------------------------------------- the model: the formula of the host before there was an Arena
def align256(v):
    return (v + 255) & ~255


def model(pieces):
    """pieces: (bytes, or None for a piece the layout leaves out) in the order taken -> (offsets with -1 for None, total)"""
    pos, offs = 0, []
    for b in pieces:
        if b is None:
            offs.append(-1)
            continue
        offs.append(pos)
        pos += align256(max(b, 4))
    return offs, pos


CLUSTER_REC, PROFILE_REC, MSA_REC, CIGAR_REC = (C.sizeof(t) for t in (_ffi.ClusterRecord, _ffi.ProfileRecord, _ffi.MsaRecord, _ffi.CigarRecord))


def cluster_pieces(mode, n, m, room, tiles, with_len):
    greedy = mode == GREEDY
    return [64, 4 * n, 4 * n, 4 * n if greedy else None, 4 * n if greedy else None, 8 * n, 4 * n, 4 * n, 4 * m, 4 * m, 4 * n if with_len else None,
            4 * tiles, 4 * tiles, CLUSTER_REC * room]


def family_pieces(n, held, n_centers):
    return [8 * MISC_WORDS, 4 * held, 4 * held, 4 * n, 4 * n, 4 * n_centers, 8 * n_centers]


def profile_pieces(n, held, n_centers, total):
    return family_pieces(n, held, n_centers) + [PROFILE_REC * n_centers, 4 * total]


def msa_plan_pieces(n, held, n_centers, n_ins):
    return family_pieces(n, held, n_centers) + [MSA_REC * n_centers, 4 * held, 4 * n_ins, 4 * n_ins]


def msa_fill_pieces(held, n_centers, nbytes, total_rows):
    return [8 * n_centers, 8 * n_centers, 4 * n_centers, 4 * total_rows, 4 * held, 4 * total_rows, nbytes]


def cigar_pieces(n):
    tiles = (n + CIGAR_TILE - 1) // CIGAR_TILE
    return [8 * CIGAR_MISC_WORDS, 4 * n, CIGAR_REC * n, 8 * (n + 1), 8 * tiles, 8 * tiles]


def cluster_cases():
    # (the tiles of the finish's compaction are a count of their own to the layout: here a tile of 64 label slots)
    return [(mode, n, m, room, (n + 63) // 64, with_len) for mode in (COMPONENTS, GREEDY) for with_len in (0, 1)
            for n, m, room in itertools.product(COUNTS, repeat=3)]


LAYOUTS = {
    "cluster": (cluster_pieces, cluster_cases),
    "profile": (profile_pieces, lambda: list(itertools.product(COUNTS, repeat=4))),
    "msa_plan": (msa_plan_pieces, lambda: list(itertools.product(COUNTS, repeat=4))),
    "msa_fill": (msa_fill_pieces, lambda: list(itertools.product(COUNTS, repeat=4))),
    "cigar": (cigar_pieces, lambda: [(n,) for n in COUNTS]),
}


def check_sizes(drv):
    (got,) = run(drv, "sizes", [])
    assert got == [CLUSTER_REC, PROFILE_REC, MSA_REC, CIGAR_REC, MISC_WORDS, MISC_WORDS, CIGAR_MISC_WORDS, GREEDY]
    assert _ffi.CLUSTER_GREEDY == GREEDY and _ffi.CLUSTER_COMPONENTS == COMPONENTS


def check_layout(drv, what):
    pieces_of, cases_of = LAYOUTS[what]
    cases = cases_of()
    got = run(drv, what, [" ".join(str(int(v)) for v in case) for case in cases])
    assert len(got) == len(cases)
    for case, line in zip(cases, got):
        pieces = pieces_of(*case)
        want, total = model(pieces)
        sized, placed, offs = line[0], line[1], line[2:]
        assert offs == want and placed == total, (what, case)
        assert sized == placed, (what, case)                       # the sizing pass ends where the placing pass does
        taken = [(o, b) for o, b in zip(offs, pieces) if b is not None]
        assert all(o % 256 == 0 for o, _ in taken) and total % 256 == 0, (what, case)
        ends = [o for o, _ in taken[1:]] + [total]
        for (o, b), end in zip(taken, ends):
            assert o + max(b, 4) <= end, (what, case)              # no piece reaches into the next, the last none beyond the arena
            if b == 0:
                assert end - o == 256, (what, case)                # a piece of no elements still has 256 bytes of its own


@pytest.mark.parametrize("what", sorted(LAYOUTS))
def test_layout(driver, what):
    check_layout(driver, what)


def test_sizes(driver):
    check_sizes(driver)


def test_the_driver_under_sanitizers(tmp_path):
    """the same checks with the driver built as a stand-alone program under AddressSanitizer and UBSan (host code only)"""
    try:
        exe = build_driver(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    except subprocess.CalledProcessError:
        print("no sanitizer runtime for this compiler: the plain driver's tests stand alone")
        return
    check_sizes(exe)
    for what in sorted(LAYOUTS):
        check_layout(exe, what)
