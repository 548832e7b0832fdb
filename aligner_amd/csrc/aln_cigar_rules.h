// aln_cigar_rules.h -- the CIGARs of a sequence set's held hits (aln_seqset_held_cigar_plan / _fill, include/aligner_hip_cigar.h): the
// two aligned strings of a hit as run-length encoded ops, and the record beside them.  Integer arithmetic only, no HIP, so that the
// kernels (aln_cigar.hip), the host and a CPU test driver decide all of it the same way.  Nothing here depends on scores.
//
//   columns    aln_report_columns(aln_len, ALN_REPORT_SKIP_SEED) = n: the seed column is never part of a CIGAR
//   op         of x = query[j], y = target[j]: both non-blank M (0), with ALN_CIGAR_EXTENDED = (7) if x == y else X (8); y blank alone
//              I (1); x blank alone D (2); both blank P (6).  SAM's numbering: the words are BAM's
//   runs       a maximal stretch of counted columns with the same op is one word length << 4 | op; column n - 1 always ends a run and
//              column n is never read, not even to look ahead
//   clips      with ALN_CIGAR_CLIPS: S (4) of start_x first, S of N - q_end last, each only when its length is not 0; q_end > N: no
//              trailing clip and one overflow.  A clip's length is held at 2^28 - 1
//   record     n_ops = runs + clips; q_end = start_x + query non-blanks, t_end = start_y + target non-blanks (64-bit sums saturated to
//              32 bits); matches: x == y != blank; block: columns that are not P.  status != ALN_OK: all zero but the status, no ops
//   offsets    hit k's words start at word sum_{j < k} n_ops_j (64 bits); entry n is the total
//   supported  every N + M + 2 of the set below 2^28, so that a run fits 28 bits: 2 * (the longest sequence) + 2 < 2^28
#pragma once
#include <stdint.h>

#include "../../include/aligner_hip_cigar.h"
#include "aln_report_rules.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define ALN_CIGAR_HD __host__ __device__
#else
#define ALN_CIGAR_HD
#endif

#define ALN_CIGAR_FLAGS (ALN_CIGAR_EXTENDED | ALN_CIGAR_CLIPS)
#define ALN_CIGAR_NO_OP 15u                       // no column: what precedes column 0 and follows column n - 1
#define ALN_CIGAR_MAX_RUN 0x0FFFFFFFu             // 28 bits
// the device's counters, 64-bit words
#define ALN_CIGAR_MISC_FAILED 0u
#define ALN_CIGAR_MISC_PADDED 1u
#define ALN_CIGAR_MISC_OVERFLOW 2u
#define ALN_CIGAR_MISC_TOTAL 3u
#define ALN_CIGAR_MISC_WORDS 4u
// the offsets are scanned in tiles of this many listed hits (the threads of aln_block_exclusive_scan)
#define ALN_CIGAR_TILE 256u

// the records' layouts, pinned at compile time (the style of aln_msa_rules.h)
#define ALN_CIGAR_PIN(name, cond) typedef char aln_cigar_pin_##name[(cond) ? 1 : -1]
ALN_CIGAR_PIN(record_size, sizeof(aln_cigar_record) == 32);
ALN_CIGAR_PIN(record_n_ops, __builtin_offsetof(aln_cigar_record, n_ops) == 0);
ALN_CIGAR_PIN(record_q_start, __builtin_offsetof(aln_cigar_record, q_start) == 4);
ALN_CIGAR_PIN(record_q_end, __builtin_offsetof(aln_cigar_record, q_end) == 8);
ALN_CIGAR_PIN(record_t_start, __builtin_offsetof(aln_cigar_record, t_start) == 12);
ALN_CIGAR_PIN(record_t_end, __builtin_offsetof(aln_cigar_record, t_end) == 16);
ALN_CIGAR_PIN(record_matches, __builtin_offsetof(aln_cigar_record, matches) == 20);
ALN_CIGAR_PIN(record_block, __builtin_offsetof(aln_cigar_record, block) == 24);
ALN_CIGAR_PIN(record_status, __builtin_offsetof(aln_cigar_record, status) == 28);
ALN_CIGAR_PIN(summary_size, sizeof(aln_cigar_summary) == 48);
ALN_CIGAR_PIN(summary_held, __builtin_offsetof(aln_cigar_summary, held) == 0);
ALN_CIGAR_PIN(summary_listed, __builtin_offsetof(aln_cigar_summary, listed) == 8);
ALN_CIGAR_PIN(summary_total_ops, __builtin_offsetof(aln_cigar_summary, total_ops) == 16);
ALN_CIGAR_PIN(summary_failed, __builtin_offsetof(aln_cigar_summary, failed) == 24);
ALN_CIGAR_PIN(summary_padded, __builtin_offsetof(aln_cigar_summary, padded) == 28);
ALN_CIGAR_PIN(summary_overflow, __builtin_offsetof(aln_cigar_summary, overflow) == 32);
ALN_CIGAR_PIN(summary_reserved, __builtin_offsetof(aln_cigar_summary, reserved) == 36);
ALN_CIGAR_PIN(ops, ALN_CIGAR_M == 0 && ALN_CIGAR_I == 1 && ALN_CIGAR_D == 2 && ALN_CIGAR_S == 4 && ALN_CIGAR_P == 6 && ALN_CIGAR_EQ == 7 && ALN_CIGAR_X == 8);

ALN_CIGAR_HD inline bool aln_cigar_flags_ok(uint32_t flags) { return (flags & ~ALN_CIGAR_FLAGS) == 0u; }

// a set whose longest sequence has max_len residues: every N + M + 2, a self pair's too, below 2^28
ALN_CIGAR_HD inline bool aln_cigar_supported(uint64_t max_len) { return 2ull * max_len + 2ull < (1ull << 28); }

ALN_CIGAR_HD inline uint64_t aln_cigar_tiles(uint64_t n) { return (n + ALN_CIGAR_TILE - 1u) / ALN_CIGAR_TILE; }

ALN_CIGAR_HD inline uint32_t aln_cigar_columns(uint32_t aln_len) { return aln_report_columns(aln_len, ALN_REPORT_SKIP_SEED); }

ALN_CIGAR_HD inline uint32_t aln_cigar_op(uint32_t x, uint32_t y, uint32_t blank, uint32_t flags)
{
    if (x == blank) return y == blank ? ALN_CIGAR_P : ALN_CIGAR_D;
    if (y == blank) return ALN_CIGAR_I;
    if (!(flags & ALN_CIGAR_EXTENDED)) return ALN_CIGAR_M;
    return x == y ? ALN_CIGAR_EQ : ALN_CIGAR_X;
}

// a run's or a clip's word (a run of counted columns is below 2^28 in a supported set; a clip's length is held there)
ALN_CIGAR_HD inline uint32_t aln_cigar_word(uint64_t length, uint32_t op)
{
    const uint32_t l = length > (uint64_t)ALN_CIGAR_MAX_RUN ? ALN_CIGAR_MAX_RUN : (uint32_t)length;
    return l << 4 | op;
}

ALN_CIGAR_HD inline uint32_t aln_cigar_saturate(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

// the clips' lengths, 0: none.  The trailing one is decided from the record's (saturated) q_end: beyond N there is none
ALN_CIGAR_HD inline uint32_t aln_cigar_lead(uint32_t start_x, uint32_t flags) { return (flags & ALN_CIGAR_CLIPS) ? start_x : 0u; }
ALN_CIGAR_HD inline uint32_t aln_cigar_trail(uint32_t q_end, uint32_t N, uint32_t flags) { return (flags & ALN_CIGAR_CLIPS) && q_end <= N ? N - q_end : 0u; }
ALN_CIGAR_HD inline bool aln_cigar_overflows(uint32_t q_end, uint32_t N, uint32_t flags) { return (flags & ALN_CIGAR_CLIPS) && q_end > N; }

ALN_CIGAR_HD inline aln_cigar_record aln_cigar_empty(int32_t status)
{
    aln_cigar_record r;
    r.n_ops = 0; r.q_start = 0; r.q_end = 0; r.t_start = 0; r.t_end = 0; r.matches = 0; r.block = 0; r.status = status;
    return r;
}

// the record of an ALN_OK hit from its counts over the counted columns: runs, query and target non-blanks, matches, P columns of n
ALN_CIGAR_HD inline aln_cigar_record aln_cigar_finish(uint32_t runs, uint32_t q_res, uint32_t t_res, uint32_t matches, uint32_t pads, uint32_t n,
                                                      uint32_t start_x, uint32_t start_y, uint32_t N, uint32_t flags)
{
    aln_cigar_record r = aln_cigar_empty(ALN_OK);
    r.q_start = start_x;
    r.q_end = aln_cigar_saturate((uint64_t)start_x + (uint64_t)q_res);
    r.t_start = start_y;
    r.t_end = aln_cigar_saturate((uint64_t)start_y + (uint64_t)t_res);
    r.matches = matches;
    r.block = n - pads;
    r.n_ops = runs + (aln_cigar_lead(start_x, flags) ? 1u : 0u) + (aln_cigar_trail(r.q_end, N, flags) ? 1u : 0u);
    return r;
}

// ---- the whole rule for one held entry, one column at a time (what the kernels' lanes do side by side).  query / target: aln_len
// bytes each, of which the first n are read.  *padded and *overflow are added to
inline aln_cigar_record aln_cigar_count(const uint8_t *query, const uint8_t *target, uint32_t aln_len, int32_t status, uint32_t start_x,
                                        uint32_t start_y, uint32_t N, uint32_t blank, uint32_t flags, uint64_t *padded, uint64_t *overflow)
{
    if (status != ALN_OK) return aln_cigar_empty(status);
    const uint32_t n = aln_cigar_columns(aln_len);
    uint32_t runs = 0, q_res = 0, t_res = 0, matches = 0, pads = 0, prev = ALN_CIGAR_NO_OP;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t x = query[j], y = target[j], op = aln_cigar_op(x, y, blank, flags);
        runs += op != prev ? 1u : 0u;
        q_res += x != blank ? 1u : 0u;
        t_res += y != blank ? 1u : 0u;
        matches += x == y && x != blank ? 1u : 0u;
        pads += op == ALN_CIGAR_P ? 1u : 0u;
        prev = op;
    }
    const aln_cigar_record r = aln_cigar_finish(runs, q_res, t_res, matches, pads, n, start_x, start_y, N, flags);
    *padded += pads;
    *overflow += aln_cigar_overflows(r.q_end, N, flags) ? 1u : 0u;
    return r;
}

// the words of a counted entry: ops has room for `room` words; returns the words the rule has (rec.n_ops for the same strings), of
// which those below `room` were written
inline uint64_t aln_cigar_write(const uint8_t *query, const uint8_t *target, uint32_t aln_len, const aln_cigar_record &rec, uint32_t N,
                                uint32_t blank, uint32_t flags, uint32_t *ops, uint64_t room)
{
    if (rec.status != ALN_OK) return 0;
    const uint32_t n = aln_cigar_columns(aln_len);
    uint64_t w = 0;
    auto put = [&](uint64_t length, uint32_t op) { if (w < room) ops[w] = aln_cigar_word(length, op); ++w; };
    if (aln_cigar_lead(rec.q_start, flags)) put(aln_cigar_lead(rec.q_start, flags), ALN_CIGAR_S);
    uint32_t s = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t op = aln_cigar_op(query[j], target[j], blank, flags);
        const uint32_t next = j + 1u < n ? aln_cigar_op(query[j + 1u], target[j + 1u], blank, flags) : ALN_CIGAR_NO_OP;
        if (next != op) { put((uint64_t)(j - s) + 1ull, op); s = j + 1u; }     // (only a run's last column writes)
    }
    if (aln_cigar_trail(rec.q_end, N, flags)) put(aln_cigar_trail(rec.q_end, N, flags), ALN_CIGAR_S);
    return w;
}

// the offsets of the listed hits from their records: off has n + 1 entries, off[n] the total.  (2^64 is out of reach: n < 2^31 records
// of less than 2^29 words each)
inline uint64_t aln_cigar_offsets(const aln_cigar_record *rec, uint64_t n, uint64_t *off)
{
    uint64_t at = 0;
    for (uint64_t k = 0; k < n; ++k) {
        if (off) off[k] = at;
        at += rec[k].n_ops;
    }
    if (off) off[n] = at;
    return at;
}
