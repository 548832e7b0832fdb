// aln_msa_rules.h -- the family alignments of a sequence set (aln_seqset_held_msa_plan / _fill, include/aligner_hip_msa.h): a centre-star
// merge of the held hits of every centre.  Integer arithmetic only, no HIP, so that the kernels (aln_msa.hip), the host and a CPU test
// driver decide all of it the same way.  Who contributes is aln_profile_decide plus "the centre has a slot" (aln_profile_rules.h).
//
//   columns    aln_report_columns(aln_len, ALN_REPORT_SKIP_SEED): the seed column is never part of a family alignment
//   position   a column whose centre code is not blank, `before` centre non-blanks in front of it: p = start + before (64-bit); it is
//              written when p < len_c, else it is an overflow column
//   insert     a column whose centre code is blank, `before` centre non-blanks in front of it, the k-th (from 0) of its maximal run: an
//              insert before p = start + before; measured and written when p <= len_c, else an overflow column.  ins[p] = the longest
//              run any contributing hit has before p (len_c + 1 entries)
//   layout     col[p] = p + ins[0] + ... + ins[p] for p in 0 .. len_c: the column of residue p, and col[len_c] = W, the width.  The
//              insert block before p is col[p] - ins[p] .. col[p] - 1; a run's k-th column is column col[p] - ins[p] + k
//   rows       row 0: the centre's residue p at col[p]; row r >= 1: the member's code of every counted column at that column's place
//   offsets    family i at byte sum_{j < i} (rows_j + 1) * width_j, its row list at entry sum_{j < i} (rows_j + 1)
#pragma once
#include <stdint.h>

#include "../../include/aligner_hip_msa.h"
#include "aln_profile_rules.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define ALN_MSA_HD __host__ __device__
#else
#define ALN_MSA_HD
#endif

// the device's counters, 64-bit words: [kind] for the kinds 0 .. 3 and the overflow as the profile call has them, then the centres
// whose width does not fit 32 bits
#define ALN_MSA_MISC_TOO_WIDE 5u
#define ALN_MSA_MISC_WORDS ALN_PROFILE_MISC_WORDS

// the records' layouts, pinned at compile time (the style of aln_profile_rules.h)
#define ALN_MSA_PIN(name, cond) typedef char aln_msa_pin_##name[(cond) ? 1 : -1]
ALN_MSA_PIN(record_size, sizeof(aln_msa_record) == 16);
ALN_MSA_PIN(record_center, __builtin_offsetof(aln_msa_record, center) == 0);
ALN_MSA_PIN(record_rows, __builtin_offsetof(aln_msa_record, rows) == 4);
ALN_MSA_PIN(record_width, __builtin_offsetof(aln_msa_record, width) == 8);
ALN_MSA_PIN(record_inserted, __builtin_offsetof(aln_msa_record, inserted) == 12);
ALN_MSA_PIN(summary_size, sizeof(aln_msa_summary) == 48);
ALN_MSA_PIN(summary_held, __builtin_offsetof(aln_msa_summary, held) == 0);
ALN_MSA_PIN(summary_contributing, __builtin_offsetof(aln_msa_summary, contributing) == 8);
ALN_MSA_PIN(summary_self_pairs, __builtin_offsetof(aln_msa_summary, self_pairs) == 16);
ALN_MSA_PIN(summary_between, __builtin_offsetof(aln_msa_summary, between_members) == 20);
ALN_MSA_PIN(summary_unlisted, __builtin_offsetof(aln_msa_summary, unlisted) == 24);
ALN_MSA_PIN(summary_overflow, __builtin_offsetof(aln_msa_summary, overflow) == 28);
ALN_MSA_PIN(summary_bytes, __builtin_offsetof(aln_msa_summary, bytes) == 32);
ALN_MSA_PIN(summary_total_rows, __builtin_offsetof(aln_msa_summary, total_rows) == 40);
ALN_MSA_PIN(misc_words, ALN_MSA_MISC_TOO_WIDE > ALN_PROFILE_MISC_OVERFLOW && ALN_MSA_MISC_TOO_WIDE < ALN_MSA_MISC_WORDS);

ALN_MSA_HD inline uint32_t aln_msa_columns(uint32_t aln_len) { return aln_report_columns(aln_len, ALN_REPORT_SKIP_SEED); }

// the centre position of a column, `before` centre non-blanks in front of it (a residue's own position; the position an insert is before)
ALN_MSA_HD inline uint64_t aln_msa_position(uint32_t start, uint32_t before) { return aln_profile_position(start, before, false); }
ALN_MSA_HD inline bool aln_msa_residue_fits(uint64_t p, uint32_t len_c) { return p < (uint64_t)len_c; }
ALN_MSA_HD inline bool aln_msa_insert_fits(uint64_t p, uint32_t len_c) { return p <= (uint64_t)len_c; }

// the column of a run's k-th column, the run before a position whose residue column is col_p and whose block is ins_p wide.  The caller
// checks k < ins_p (true for a plan measured over the same strings) and the result against the width
ALN_MSA_HD inline uint64_t aln_msa_insert_column(uint32_t col_p, uint32_t ins_p, uint32_t k) { return (uint64_t)col_p - (uint64_t)ins_p + (uint64_t)k; }

// ---- the whole rule for one contributing hit, one column at a time (what the kernels' lanes do side by side).  center / member: the
// two aligned strings; start: the centre's start coordinate.  Measure: ins has len_c + 1 entries; returns the overflow columns
inline uint64_t aln_msa_measure(const uint8_t *center, uint32_t aln_len, uint32_t start, uint32_t blank, uint32_t len_c, uint32_t *ins)
{
    const uint32_t n = aln_msa_columns(aln_len);
    uint64_t overflow = 0;
    uint32_t before = 0, run = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const uint64_t p = aln_msa_position(start, before);
        if (center[j] != blank) {
            if (!aln_msa_residue_fits(p, len_c)) ++overflow;
            ++before;
            run = 0;
            continue;
        }
        ++run;
        if (!aln_msa_insert_fits(p, len_c)) { ++overflow; continue; }
        if ((j + 1u == n || center[j + 1u] != blank) && ins[p] < run) ins[p] = run;        // (only a run's last column measures it)
    }
    return overflow;
}

// ins -> col (len_c + 1 entries each; col may be null); returns the width in 64 bits
inline uint64_t aln_msa_layout(const uint32_t *ins, uint32_t len_c, uint32_t *col)
{
    uint64_t sum = 0;
    for (uint64_t p = 0; p <= len_c; ++p) {
        sum += ins[p];
        if (col) col[p] = (uint32_t)(p + sum);
    }
    return (uint64_t)len_c + sum;
}

// row 0 of a family: `row` has `width` bytes, filled with the blank code before
inline void aln_msa_center_row(const uint8_t *residues, uint32_t len_c, const uint32_t *col, uint8_t *row, uint64_t width)
{
    for (uint32_t p = 0; p < len_c; ++p)
        if (col[p] < width) row[col[p]] = residues[p];
}

// a member's row: `row` has `width` bytes, filled with the blank code before
inline void aln_msa_member_row(const uint8_t *center, const uint8_t *member, uint32_t aln_len, uint32_t start, uint32_t blank, uint32_t len_c,
                               const uint32_t *ins, const uint32_t *col, uint8_t *row, uint64_t width)
{
    const uint32_t n = aln_msa_columns(aln_len);
    uint32_t before = 0, run = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const uint64_t p = aln_msa_position(start, before);
        uint64_t at;
        if (center[j] != blank) {
            ++before;
            run = 0;
            if (!aln_msa_residue_fits(p, len_c)) continue;
            at = col[p];
        } else {
            const uint32_t k = run++;
            if (!aln_msa_insert_fits(p, len_c) || k >= ins[p]) continue;
            at = aln_msa_insert_column(col[p], ins[p], k);
        }
        if (at < width) row[at] = member[j];
    }
}

// the offsets of the families from their records: byte_off / row_off have n entries (may be null).  False when a total leaves 64 bits
inline bool aln_msa_offsets(const aln_msa_record *rec, uint64_t n, uint64_t *byte_off, uint64_t *row_off, uint64_t *bytes, uint64_t *total_rows)
{
    uint64_t b = 0, r = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (byte_off) byte_off[i] = b;
        if (row_off) row_off[i] = r;
        const uint64_t rows = (uint64_t)rec[i].rows + 1ull, size = rows * (uint64_t)rec[i].width;      // (33 + 32 bits)
        if (size > ~b) return false;
        b += size;
        r += rows;
    }
    *bytes = b;
    *total_rows = r;
    return true;
}
