// aln_arena_rules.h -- the device arenas of the calls on a sequence set's held hits (aln_host.hip): the tables of one call carved out of
// one allocation, every layout written once.  Plain C++, no HIP and no device code: the host and a CPU test driver place every piece
// the same way (tests/test_arena_rules_cpu.py holds the formula against a model).
//
//   piece      `count` elements of T take align256(max(sizeof(T) * count, 4)) bytes: every piece starts on a multiple of 256, and a
//              piece of no elements still has an address of its own
//   sizing     a null base places nothing: take() returns null and bytes() is what the same takes need.  A call sizes its arena with
//              a null base, ensures the allocation and carves again with the real one
//   re-carve   a fill carves the plan's arena again from the counts the plan kept and finds the plan's tables: a layout depends on
//              its counts alone
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "aln_cluster_rules.h"
#include "aln_profile_rules.h"
#include "aln_msa_rules.h"
#include "aln_cigar_rules.h"

static inline uint64_t align256(uint64_t v) { return (v + 255) & ~255ull; }

struct Arena {
    uint8_t *base;
    size_t pos = 0;
    explicit Arena(uint8_t *b) : base(b) {}
    template <class T> T *take(uint64_t count)
    {
        T *p = base ? reinterpret_cast<T *>(base + pos) : nullptr;
        const uint64_t bytes = sizeof(T) * count;
        pos += (size_t)align256(bytes < 4 ? 4 : bytes);
        return p;
    }
    size_t bytes() const { return pos; }
};

// ---- clusters of an edge list (aln_cluster.hip): n label slots, m edges, room records, `tiles` tiles of the finish's compaction
// (aln_cluster_tiles(n)); aux1 / aux2 only in greedy mode, len only when the caller brings lengths
struct ClusterBufs {
    uint32_t *misc = nullptr, *label = nullptr, *aux0 = nullptr, *aux1 = nullptr, *aux2 = nullptr, *size = nullptr, *cedges = nullptr;
    uint64_t *key = nullptr;
    uint32_t *ea = nullptr, *eb = nullptr, *len = nullptr, *tile_count = nullptr, *tile_off = nullptr;
    aln_cluster_record *rec = nullptr;
};
static inline size_t cluster_carve(uint8_t *base, uint32_t mode, uint64_t n, uint64_t m, uint64_t room, uint64_t tiles, bool with_len, ClusterBufs *out)
{
    Arena ar(base);
    ClusterBufs b;
    b.misc = ar.take<uint32_t>(16);
    b.label = ar.take<uint32_t>(n);
    b.aux0 = ar.take<uint32_t>(n);
    if (mode == ALN_CLUSTER_GREEDY) {
        b.aux1 = ar.take<uint32_t>(n);
        b.aux2 = ar.take<uint32_t>(n);
    }
    b.key = ar.take<uint64_t>(n);
    b.size = ar.take<uint32_t>(n);
    b.cedges = ar.take<uint32_t>(n);
    b.ea = ar.take<uint32_t>(m);
    b.eb = ar.take<uint32_t>(m);
    if (with_len) b.len = ar.take<uint32_t>(n);
    b.tile_off = ar.take<uint32_t>(tiles);
    b.tile_count = ar.take<uint32_t>(tiles);
    b.rec = ar.take<aln_cluster_record>(room);
    if (out) *out = b;
    return ar.bytes();
}

// ---- what profiles and the MSA plan share (aln_profile.hip, aln_msa.hip): the counters, the held hits' endpoints, the labelling, the
// centres and their slots and offsets.  Both layouts begin with these pieces, a record table of their own after them
struct FamilyBufs {
    unsigned long long *misc = nullptr;
    uint32_t *hit_q = nullptr, *hit_t = nullptr, *label = nullptr, *slot_of = nullptr, *centers = nullptr;
    uint64_t *off = nullptr;
};
static inline void family_carve(Arena &ar, uint64_t n, uint64_t held, uint64_t n_centers, FamilyBufs &b)
{
    b.misc = ar.take<unsigned long long>(ALN_PROFILE_MISC_WORDS);
    b.hit_q = ar.take<uint32_t>(held);
    b.hit_t = ar.take<uint32_t>(held);
    b.label = ar.take<uint32_t>(n);
    b.slot_of = ar.take<uint32_t>(n);
    b.centers = ar.take<uint32_t>(n_centers);
    b.off = ar.take<uint64_t>(n_centers);
}

// ---- profiles of a set's families: the shared pieces, the records and the call's output of `total` elements
struct ProfileBufs : FamilyBufs {
    aln_profile_record *rec = nullptr;
    uint32_t *out = nullptr;
};
static inline size_t profile_carve(uint8_t *base, uint64_t n, uint64_t held, uint64_t n_centers, uint64_t total, ProfileBufs *out)
{
    Arena ar(base);
    ProfileBufs b;
    family_carve(ar, n, held, n_centers, b);
    b.rec = ar.take<aln_profile_record>(n_centers);
    b.out = ar.take<uint32_t>(total);
    if (out) *out = b;
    return ar.bytes();
}

// ---- the plan of the family alignments: the shared pieces (off: where a centre's entries of ins / col start), the records, the
// held hits' marks and the n_ins insert widths and columns
struct MsaPlanBufs : FamilyBufs {
    aln_msa_record *rec = nullptr;
    uint32_t *mark = nullptr, *ins = nullptr, *col = nullptr;
};
static inline size_t msa_plan_carve(uint8_t *base, uint64_t n, uint64_t held, uint64_t n_centers, uint64_t n_ins, MsaPlanBufs *out)
{
    Arena ar(base);
    MsaPlanBufs b;
    family_carve(ar, n, held, n_centers, b);
    b.rec = ar.take<aln_msa_record>(n_centers);
    b.mark = ar.take<uint32_t>(held);
    b.ins = ar.take<uint32_t>(n_ins);
    b.col = ar.take<uint32_t>(n_ins);
    if (out) *out = b;
    return ar.bytes();
}

// ---- the fill of the family alignments: its tables and its output, an arena of their own (sized when the plan's totals are known)
struct MsaFillBufs {
    uint64_t *byte_off = nullptr, *row_off = nullptr;
    uint32_t *taken = nullptr, *list = nullptr, *hit_row = nullptr, *row_hit = nullptr;
    uint8_t *out = nullptr;
};
static inline size_t msa_fill_carve(uint8_t *base, uint64_t held, uint64_t n_centers, uint64_t bytes, uint64_t total_rows, MsaFillBufs *out)
{
    Arena ar(base);
    MsaFillBufs b;
    b.byte_off = ar.take<uint64_t>(n_centers);
    b.row_off = ar.take<uint64_t>(n_centers);
    b.taken = ar.take<uint32_t>(n_centers);
    b.list = ar.take<uint32_t>(total_rows);
    b.hit_row = ar.take<uint32_t>(held);
    b.row_hit = ar.take<uint32_t>(total_rows);
    b.out = ar.take<uint8_t>(bytes);
    if (out) *out = b;
    return ar.bytes();
}

// ---- the plan of the CIGARs: the counters, the n listed positions, their records, the n + 1 offsets and the scan's tiles
struct CigarBufs {
    unsigned long long *misc = nullptr;
    uint32_t *list = nullptr;
    aln_cigar_record *rec = nullptr;
    uint64_t *off = nullptr, *tile_sum = nullptr, *tile_off = nullptr;
};
static inline size_t cigar_carve(uint8_t *base, uint64_t n, CigarBufs *out)
{
    Arena ar(base);
    CigarBufs b;
    b.misc = ar.take<unsigned long long>(ALN_CIGAR_MISC_WORDS);
    b.list = ar.take<uint32_t>(n);
    b.rec = ar.take<aln_cigar_record>(n);
    b.off = ar.take<uint64_t>(n + 1);
    b.tile_sum = ar.take<uint64_t>(aln_cigar_tiles(n));
    b.tile_off = ar.take<uint64_t>(aln_cigar_tiles(n));
    if (out) *out = b;
    return ar.bytes();
}
