// aln_profile_rules.h -- the profiles of a sequence set's families (aln_seqset_held_profiles, include/aligner_hip_profile.h): which
// held hits contribute to which centre, where a column of the aligned strings lies on the centre, and which row it is counted in.
// Integer arithmetic only, no HIP, so that the kernel (aln_profile.hip), the host and a CPU test driver decide all of it the same way.
//
//   decide     an ALN_OK (and, with a filter, kept) hit (q, t) with labels lq, lt: q == t SELF; lq != lt or lq == NONE: SKIP, counted
//              nowhere; neither q nor t equals the label: BETWEEN; else the end that equals the label is the centre.  The caller
//              turns a centre without a slot into UNLISTED.  A label is compared, never used as an index
//   columns    aln_report_columns(aln_len, flags); the seed column is column aln_len - 1 when it is among them
//   position   of a column whose centre code is not blank, `before` non-blank centre codes in front of it: start + before; the seed
//              column repeats the end cell's residue and sits where the non-blank in front of it sits, start + before - 1 (start when
//              there is none).  64-bit, so that nothing wraps before it is compared with len[c]
//   row        mc < n_codes: mc; mc == blank: n_codes; else n_codes + 1 (in this order: a blank code below n_codes is a residue row)
//   layout     profile i at element sum_{j < i} (n_codes + 2) * len[centers[j]], row-major [row][position]
#pragma once
#include <stdint.h>

#include "../../include/aligner_hip_profile.h"
#include "aln_report_rules.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define ALN_PROFILE_HD __host__ __device__
#else
#define ALN_PROFILE_HD
#endif

enum aln_profile_kind {
    ALN_PROFILE_COUNTS = 0,       // contributes: *center and *center_is_query are set
    ALN_PROFILE_SELF = 1,
    ALN_PROFILE_BETWEEN = 2,
    ALN_PROFILE_UNLISTED = 3,     // (the caller's: the centre has no slot)
    ALN_PROFILE_SKIP = 4
};
#define ALN_PROFILE_NO_COLUMN 0xFFFFFFFFu
// the device's counters, 64-bit words: [kind] for the kinds 0 .. 3, then the overflow
#define ALN_PROFILE_MISC_OVERFLOW 4u
#define ALN_PROFILE_MISC_WORDS 8u

// the records' layouts, pinned at compile time (the style of aln_report_rules.h)
#define ALN_PROFILE_PIN(name, cond) typedef char aln_profile_pin_##name[(cond) ? 1 : -1]
ALN_PROFILE_PIN(record_size, sizeof(aln_profile_record) == 16);
ALN_PROFILE_PIN(record_center, __builtin_offsetof(aln_profile_record, center) == 0);
ALN_PROFILE_PIN(record_hits, __builtin_offsetof(aln_profile_record, hits) == 4);
ALN_PROFILE_PIN(record_matched, __builtin_offsetof(aln_profile_record, matched) == 8);
ALN_PROFILE_PIN(record_deleted, __builtin_offsetof(aln_profile_record, deleted) == 12);
ALN_PROFILE_PIN(summary_size, sizeof(aln_profile_summary) == 48);
ALN_PROFILE_PIN(summary_held, __builtin_offsetof(aln_profile_summary, held) == 0);
ALN_PROFILE_PIN(summary_contributing, __builtin_offsetof(aln_profile_summary, contributing) == 8);
ALN_PROFILE_PIN(summary_self_pairs, __builtin_offsetof(aln_profile_summary, self_pairs) == 16);
ALN_PROFILE_PIN(summary_between, __builtin_offsetof(aln_profile_summary, between_members) == 20);
ALN_PROFILE_PIN(summary_unlisted, __builtin_offsetof(aln_profile_summary, unlisted) == 24);
ALN_PROFILE_PIN(summary_overflow, __builtin_offsetof(aln_profile_summary, overflow) == 28);
ALN_PROFILE_PIN(summary_elements, __builtin_offsetof(aln_profile_summary, elements) == 32);
ALN_PROFILE_PIN(summary_reserved, __builtin_offsetof(aln_profile_summary, reserved) == 40);
ALN_PROFILE_PIN(skip_seed, ALN_PROFILE_SKIP_SEED == ALN_REPORT_SKIP_SEED);

ALN_PROFILE_HD inline bool aln_profile_codes_ok(uint32_t n_codes) { return n_codes >= 1u && n_codes <= ALN_PROFILE_MAX_CODES; }
ALN_PROFILE_HD inline uint32_t aln_profile_rows(uint32_t n_codes) { return n_codes + 2u; }

ALN_PROFILE_HD inline uint32_t aln_profile_decide(uint32_t q, uint32_t t, uint32_t label_q, uint32_t label_t, uint32_t *center, uint32_t *center_is_query)
{
    if (q == t) return ALN_PROFILE_SELF;
    if (label_q != label_t || label_q == ALN_CLUSTER_NONE) return ALN_PROFILE_SKIP;
    if (q != label_q && t != label_q) return ALN_PROFILE_BETWEEN;
    *center_is_query = q == label_q ? 1u : 0u;       // (q != t: exactly one of them)
    *center = label_q;
    return ALN_PROFILE_COUNTS;
}

// the seed column among the aln_len columns of a hit, ALN_PROFILE_NO_COLUMN when it is not counted
ALN_PROFILE_HD inline uint32_t aln_profile_seed_column(uint32_t aln_len, uint32_t flags)
{
    return (flags & ALN_PROFILE_SKIP_SEED) || aln_len == 0u ? ALN_PROFILE_NO_COLUMN : aln_len - 1u;
}

ALN_PROFILE_HD inline uint64_t aln_profile_position(uint32_t start, uint32_t before, bool seed)
{
    return (uint64_t)start + (uint64_t)before - (seed && before ? 1ull : 0ull);
}

ALN_PROFILE_HD inline uint32_t aln_profile_row(uint32_t mc, uint32_t blank, uint32_t n_codes)
{
    return mc < n_codes ? mc : mc == blank ? n_codes : n_codes + 1u;
}

// what one contributing hit adds besides the profile's elements
struct aln_profile_tally { uint32_t matched, deleted; uint64_t overflow; };

// the whole rule for one contributing hit, one column at a time (what the kernel's lanes do side by side): center / member are the two
// aligned strings, start the centre's start coordinate, profile the centre's (n_codes + 2) x len_c elements
inline aln_profile_tally aln_profile_count(const uint8_t *center, const uint8_t *member, uint32_t aln_len, uint32_t start, uint32_t flags,
                                           uint32_t blank, uint32_t n_codes, uint32_t len_c, uint32_t *profile)
{
    aln_profile_tally a = {0u, 0u, 0ull};
    const uint32_t n = aln_report_columns(aln_len, flags), seed = aln_profile_seed_column(aln_len, flags);
    uint32_t before = 0;
    for (uint32_t j = 0; j < n; ++j) {
        if (center[j] == blank) continue;
        const uint64_t pos = aln_profile_position(start, before, j == seed);
        ++before;
        if (pos >= len_c) { ++a.overflow; continue; }
        const uint32_t row = aln_profile_row(member[j], blank, n_codes);
        profile[(uint64_t)row * len_c + pos] += 1u;
        a.matched += row < n_codes ? 1u : 0u;
        a.deleted += row == n_codes ? 1u : 0u;
    }
    return a;
}

// the layout: offsets[i] = the first element of profile i (n_centers entries, may be null); returns the total.  len: the set's lengths
template <class Len>
inline uint64_t aln_profile_layout(const Len *len, const uint32_t *centers, uint64_t n_centers, uint32_t n_codes, uint64_t *offsets)
{
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_centers; ++i) {
        if (offsets) offsets[i] = total;
        total += (uint64_t)aln_profile_rows(n_codes) * (uint64_t)len[centers[i]];
    }
    return total;
}

// centres strictly ascending and below n_seqs
inline bool aln_profile_centers_ok(const uint32_t *centers, uint64_t n_centers, uint64_t n_seqs)
{
    for (uint64_t i = 0; i < n_centers; ++i)
        if (centers[i] >= n_seqs || (i && centers[i] <= centers[i - 1])) return false;
    return true;
}
