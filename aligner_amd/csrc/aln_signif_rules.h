// aln_signif_rules.h -- the per-hit reduction of aln_seqset_held_significance (include/aligner_hip.h): what a hit's shuffled copies
// leave behind as one 48-byte record, and the order in which their scores are added.  Plain arithmetic, no HIP, so that the reduce
// kernel (aln_signif.hip), the host and a CPU test driver produce the same bits -- also for real-valued schemes, where the order of
// a floating-point sum shows.
//
//   copy      copy s of a hit has an f and a status (its aln_pair_result).  A copy with status ALN_OK is TAKEN: sum += f,
//             sum_sq += f * f (the product rounded, then added: no fma), f_max = f if f > f_max, ++n_ok, and ++n_ge if f >= f_hit
//             (plain IEEE compares).  A failed copy only competes for (first_bad, status): the lowest failed copy number and its status.
//   order     64 partial accumulators; accumulator l takes copies l, l + 64, l + 128, ... in ascending order.  Then they are folded:
//             for w = 32, 16, 8, 4, 2, 1: a[l] = a[l] (+) a[l + w] for l < w, where (+) adds the sums and counts (left operand first),
//             keeps the larger f_max and the lower first_bad with its status.  The record is a[0].
//   empty     an accumulator that took no copy: +0.0 / +0.0 / -inf / 0 / 0 / ALN_OK / 0xffffffff (the record's reserved word is 0)
#pragma once
#include <stdint.h>

#include "../../include/aligner_hip.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define ALN_SIGNIF_HD __host__ __device__
#else
#define ALN_SIGNIF_HD
#endif

#define ALN_SIGNIF_LANES 64u
#define ALN_SIGNIF_NONE 0xffffffffu

// the record's layout, pinned at compile time (the style of tests/abi_harness.c)
#define ALN_SIGNIF_PIN(name, cond) typedef char aln_signif_pin_##name[(cond) ? 1 : -1]
ALN_SIGNIF_PIN(size, sizeof(aln_signif_record) == 48);
ALN_SIGNIF_PIN(sum, __builtin_offsetof(aln_signif_record, sum) == 0);
ALN_SIGNIF_PIN(sum_sq, __builtin_offsetof(aln_signif_record, sum_sq) == 8);
ALN_SIGNIF_PIN(f_max, __builtin_offsetof(aln_signif_record, f_max) == 16);
ALN_SIGNIF_PIN(n_ok, __builtin_offsetof(aln_signif_record, n_ok) == 24);
ALN_SIGNIF_PIN(n_ge, __builtin_offsetof(aln_signif_record, n_ge) == 28);
ALN_SIGNIF_PIN(status, __builtin_offsetof(aln_signif_record, status) == 32);
ALN_SIGNIF_PIN(first_bad, __builtin_offsetof(aln_signif_record, first_bad) == 36);
ALN_SIGNIF_PIN(reserved, __builtin_offsetof(aln_signif_record, reserved) == 40);

ALN_SIGNIF_HD inline aln_signif_record aln_signif_empty(void)
{
    aln_signif_record a;
    a.sum = 0.0; a.sum_sq = 0.0; a.f_max = -__builtin_inf();
    a.n_ok = 0; a.n_ge = 0; a.status = ALN_OK; a.first_bad = ALN_SIGNIF_NONE; a.reserved = 0;
    return a;
}

// copy s into its accumulator
ALN_SIGNIF_HD inline void aln_signif_take(aln_signif_record *a, uint32_t s, double f, int32_t status, double f_hit)
{
    if (status == ALN_OK) {
        const double sq = f * f;
        a->sum = a->sum + f;
        a->sum_sq = a->sum_sq + sq;
        if (f > a->f_max) a->f_max = f;
        a->n_ok += 1u;
        if (f >= f_hit) a->n_ge += 1u;
    } else if (s < a->first_bad) {
        a->first_bad = s; a->status = status;
    }
}

// a (+) b
ALN_SIGNIF_HD inline aln_signif_record aln_signif_fold(aln_signif_record a, aln_signif_record b)
{
    a.sum = a.sum + b.sum;
    a.sum_sq = a.sum_sq + b.sum_sq;
    if (b.f_max > a.f_max) a.f_max = b.f_max;
    a.n_ok += b.n_ok;
    a.n_ge += b.n_ge;
    if (b.first_bad < a.first_bad) { a.first_bad = b.first_bad; a.status = b.status; }
    return a;
}

// the whole rule, one accumulator at a time (what the reduce kernel's lanes do side by side).  f / status: entry s of arrays with the
// given strides in bytes (the copies' aln_pair_result entries, or plain arrays)
inline aln_signif_record aln_signif_reduce(const void *f, uint64_t f_stride, const void *status, uint64_t status_stride, uint32_t per_pair,
                                           double f_hit)
{
    aln_signif_record a[ALN_SIGNIF_LANES];
    for (uint32_t l = 0; l < ALN_SIGNIF_LANES; ++l) {
        a[l] = aln_signif_empty();
        for (uint32_t s = l; s < per_pair; s += ALN_SIGNIF_LANES) {
            double v; int32_t st;
            __builtin_memcpy(&v, (const char *)f + (uint64_t)s * f_stride, 8);
            __builtin_memcpy(&st, (const char *)status + (uint64_t)s * status_stride, 4);
            aln_signif_take(&a[l], s, v, st, f_hit);
        }
    }
    for (uint32_t w = ALN_SIGNIF_LANES / 2; w >= 1u; w >>= 1)
        for (uint32_t l = 0; l < w; ++l) a[l] = aln_signif_fold(a[l], a[l + w]);
    return a[0];
}
