// aln_report_rules.h -- the report of a held hit (aln_seqset_held_report / aln_seqset_held_filter, include/aligner_hip.h): which class
// a column of the two aligned strings falls into, what is counted, and which reports a filter keeps.  Integer counting and plain IEEE
// compares, no HIP, so that the kernel (aln_report.hip), the host and a CPU test driver decide all of it the same way.
//
//   strings    x = query[j], y = target[j], j = 0 .. aln_len - 1, as held_strings returns them; blank = params->blank_code
//   columns    all aln_len, or with ALN_REPORT_SKIP_SEED aln_len - 1 (0 for aln_len 0): the last column is the end cell's pair the
//              reference's traceback seeds both strings with before the walk (simple/mod.rs:102-105, 213-216)
//   class      the midline of Alignment::get_alignment (alignment.rs:25-42), restated: IDENTICAL x == y and x != blank; POSITIVE both
//              non-blank, x != y and S[y][x] >= 0.0 (0.0 and -0.0 are, a NaN is not; a code beyond the matrix is not); MISMATCH both
//              non-blank, x != y, not positive; Q_GAP x == blank, y != blank; T_GAP y == blank, x != blank; BLANK both blank
//              (counted in `columns` only)
//   opens      a Q_GAP column j with j == 0 or column j - 1 not Q_GAP is a q_gap_open; T_GAP alike
//   table      the rule reads one bit of S per entry: bit t * cols + q of a table of rows * cols bits (<= ALN_REPORT_MAX_BITS), set iff
//              matrix[t * row_stride + q] >= 0.0
//   filter     kept iff status == ALN_OK, columns >= min_columns, (double)identical >= min_identity * (double)columns,
//              (double)(columns - q_gap) >= min_q_cover * (double)N, (double)(columns - t_gap) >= min_t_cover * (double)M: one
//              multiplication and one compare each (no fma: -ffp-contract=off); a NaN threshold keeps nothing
#pragma once
#include <stdint.h>

#include "../../include/aligner_hip.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define ALN_REPORT_HD __host__ __device__
#else
#define ALN_REPORT_HD
#endif

#define ALN_REPORT_MAX_BITS 8192u                 // rows * cols: the bound of aln_transform_matrices
#define ALN_REPORT_MAX_WORDS (ALN_REPORT_MAX_BITS / 32u)

enum aln_report_class {
    ALN_REPORT_IDENTICAL = 0, ALN_REPORT_POSITIVE = 1, ALN_REPORT_MISMATCH = 2, ALN_REPORT_Q_GAP = 3, ALN_REPORT_T_GAP = 4,
    ALN_REPORT_BLANK = 5,
    ALN_REPORT_NONE = 6                           // no column: what precedes column 0
};

// the records' layouts, pinned at compile time (the style of tests/abi_harness.c)
#define ALN_REPORT_PIN(name, cond) typedef char aln_report_pin_##name[(cond) ? 1 : -1]
ALN_REPORT_PIN(size, sizeof(aln_hit_report) == 40);
ALN_REPORT_PIN(columns, __builtin_offsetof(aln_hit_report, columns) == 0);
ALN_REPORT_PIN(identical, __builtin_offsetof(aln_hit_report, identical) == 4);
ALN_REPORT_PIN(positive, __builtin_offsetof(aln_hit_report, positive) == 8);
ALN_REPORT_PIN(mismatch, __builtin_offsetof(aln_hit_report, mismatch) == 12);
ALN_REPORT_PIN(q_gap, __builtin_offsetof(aln_hit_report, q_gap) == 16);
ALN_REPORT_PIN(t_gap, __builtin_offsetof(aln_hit_report, t_gap) == 20);
ALN_REPORT_PIN(q_gap_open, __builtin_offsetof(aln_hit_report, q_gap_open) == 24);
ALN_REPORT_PIN(t_gap_open, __builtin_offsetof(aln_hit_report, t_gap_open) == 28);
ALN_REPORT_PIN(status, __builtin_offsetof(aln_hit_report, status) == 32);
ALN_REPORT_PIN(reserved, __builtin_offsetof(aln_hit_report, reserved) == 36);
ALN_REPORT_PIN(filter_size, sizeof(aln_hit_filter) == 32);
ALN_REPORT_PIN(min_identity, __builtin_offsetof(aln_hit_filter, min_identity) == 0);
ALN_REPORT_PIN(min_q_cover, __builtin_offsetof(aln_hit_filter, min_q_cover) == 8);
ALN_REPORT_PIN(min_t_cover, __builtin_offsetof(aln_hit_filter, min_t_cover) == 16);
ALN_REPORT_PIN(min_columns, __builtin_offsetof(aln_hit_filter, min_columns) == 24);
ALN_REPORT_PIN(filter_reserved, __builtin_offsetof(aln_hit_filter, reserved) == 28);

ALN_REPORT_HD inline uint32_t aln_report_words(uint32_t rows, uint32_t cols) { return (rows * cols + 31u) / 32u; }

// the table of a scheme (host): bits[] holds aln_report_words(rows, cols) words; rows * cols <= ALN_REPORT_MAX_BITS
inline void aln_report_table(const double *matrix, uint32_t rows, uint32_t cols, int64_t row_stride, uint32_t *bits)
{
    const uint32_t words = aln_report_words(rows, cols);
    for (uint32_t w = 0; w < words; ++w) bits[w] = 0u;
    for (uint32_t t = 0; t < rows; ++t)
        for (uint32_t q = 0; q < cols; ++q) {
            const uint32_t b = t * cols + q;
            if (matrix[(int64_t)t * row_stride + (int64_t)q] >= 0.0) bits[b >> 5] |= 1u << (b & 31u);
        }
}

// columns counted of aln_len
ALN_REPORT_HD inline uint32_t aln_report_columns(uint32_t aln_len, uint32_t flags)
{
    return (flags & ALN_REPORT_SKIP_SEED) && aln_len ? aln_len - 1u : aln_len;
}

ALN_REPORT_HD inline uint32_t aln_report_class_of(uint32_t x, uint32_t y, uint32_t blank, const uint32_t *bits, uint32_t rows, uint32_t cols)
{
    if (x == blank) return y == blank ? ALN_REPORT_BLANK : ALN_REPORT_Q_GAP;
    if (y == blank) return ALN_REPORT_T_GAP;
    if (x == y) return ALN_REPORT_IDENTICAL;
    if (x >= cols || y >= rows) return ALN_REPORT_MISMATCH;
    const uint32_t b = y * cols + x;
    return (bits[b >> 5] >> (b & 31u)) & 1u ? ALN_REPORT_POSITIVE : ALN_REPORT_MISMATCH;
}

ALN_REPORT_HD inline aln_hit_report aln_report_empty(int32_t status)
{
    aln_hit_report a;
    a.columns = 0; a.identical = 0; a.positive = 0; a.mismatch = 0; a.q_gap = 0; a.t_gap = 0; a.q_gap_open = 0; a.t_gap_open = 0;
    a.status = status; a.reserved = 0;
    return a;
}

// one column of class c whose predecessor has class prev (ALN_REPORT_NONE in front of column 0)
ALN_REPORT_HD inline void aln_report_take(aln_hit_report *a, uint32_t c, uint32_t prev)
{
    a->columns += 1u;
    a->identical += c == ALN_REPORT_IDENTICAL ? 1u : 0u;
    a->positive += c == ALN_REPORT_POSITIVE ? 1u : 0u;
    a->mismatch += c == ALN_REPORT_MISMATCH ? 1u : 0u;
    a->q_gap += c == ALN_REPORT_Q_GAP ? 1u : 0u;
    a->t_gap += c == ALN_REPORT_T_GAP ? 1u : 0u;
    a->q_gap_open += c == ALN_REPORT_Q_GAP && prev != ALN_REPORT_Q_GAP ? 1u : 0u;
    a->t_gap_open += c == ALN_REPORT_T_GAP && prev != ALN_REPORT_T_GAP ? 1u : 0u;
}

// a (+) b: the counts added; status and reserved are a's
ALN_REPORT_HD inline aln_hit_report aln_report_fold(aln_hit_report a, const aln_hit_report &b)
{
    a.columns += b.columns; a.identical += b.identical; a.positive += b.positive; a.mismatch += b.mismatch;
    a.q_gap += b.q_gap; a.t_gap += b.t_gap; a.q_gap_open += b.q_gap_open; a.t_gap_open += b.t_gap_open;
    return a;
}

// the whole rule for one held entry, one column at a time (what the kernel's lanes do side by side)
inline aln_hit_report aln_report_count(const uint8_t *query, const uint8_t *target, uint32_t aln_len, int32_t status, uint32_t flags,
                                       uint32_t blank, const uint32_t *bits, uint32_t rows, uint32_t cols)
{
    aln_hit_report a = aln_report_empty(status);
    if (status != ALN_OK) return a;
    const uint32_t n = aln_report_columns(aln_len, flags);
    uint32_t prev = ALN_REPORT_NONE;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t c = aln_report_class_of(query[j], target[j], blank, bits, rows, cols);
        aln_report_take(&a, c, prev);
        prev = c;
    }
    return a;
}

// the filter: N, M the lengths of the entry's query and target sequences
ALN_REPORT_HD inline bool aln_report_keep(const aln_hit_report &r, const aln_hit_filter &f, uint32_t N, uint32_t M)
{
    if (r.status != ALN_OK || !(r.columns >= f.min_columns)) return false;
    const double columns = (double)r.columns;
    const double need_id = f.min_identity * columns;
    const double need_q = f.min_q_cover * (double)N;
    const double need_t = f.min_t_cover * (double)M;
    return (double)r.identical >= need_id && (double)(r.columns - r.q_gap) >= need_q && (double)(r.columns - r.t_gap) >= need_t;
}
