// aln_transform_rules.h -- the matrix re-estimation step of the heuristic loop (transform_matrix, aligner-helpers/src/matrices/mod.rs:19-68,
// mirrored in aligner_amd/heuristic.py) as plain f64 arithmetic with a FIXED order of operations, so that aln_transform_matrices
// (aln_pairset.hip, host code, no GPU), the Python mirror and a pure-Python restatement (tests/transform_ref.py) give the same bits.
// Compiled without contraction (-ffp-contract=off): every product and sum below is rounded on its own.
//
//   sum       every reduction runs over the rows * cols elements in row-major order, in the order of numpy's contiguous f64 sum:
//               n < 8        r = 0.0; r += a[i] in turn
//               n <= 128     eight running sums r[j] = a[j], r[j] += a[i + j] for i = 8, 16, ... while i + 8 <= n;
//                            ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); then the tail a[i] .. a[n - 1] is added in turn
//               n > 128      sum(a, h) + sum(a + h, n - h) with h = n / 2 rounded down to a multiple of 8
//             and the reduction's result is 0.0 + that sum.  Matrices of more than ALN_TRANSFORM_MAX_ENTRIES elements are refused
//             (numpy sums larger arrays buffer by buffer: another order).
//   p         p[t][q] = frequencies[t] * (1.0 / cols)
//   scalars   p2 = sum(p * p); k0 = sum(p * m); a = (kd - k0) / p2; b = kd / p2; base = m + p * (a - b); den = sum(base * base);
//             a1 = ((2.0 * b) * sum(p * base)) / den; a0 = ((b * b) * p2 - r_squared) / den
//   roots     of x^2 + a1 x + a0, the branches of roots 0.0.7's find_roots_quadratic with a2 = 1.0: disc = a1 * a1 - (4.0 * 1.0) * a0;
//             disc < 0: none (status ALN_TRANSFORM_NO_ROOT, the reference's WrongMatrixSpecified); disc == 0: one, -a1 / 2.0;
//             otherwise sq = sqrt(disc), (same, diff) = a1 < 0 ? (-a1 + sq, -a1 - sq) : (-a1 - sq, -a1 + sq) and
//               |same| > 2:  x1 = (2.0 * a0) / same; x2 = |diff| > 2 ? (2.0 * a0) / diff : same / 2.0
//               otherwise:   x1 = diff / 2.0; x2 = same / 2.0
//             in ascending order ((x1, x2) if x1 < x2, else (x2, x1)): comparisons with a NaN are false, as in the mirror.
//   result    one root x: p * b + x * base.  Two roots lo, hi: lo > 0 and hi < 0 -> lo's; lo < 0 and hi > 0 -> hi's; otherwise both
//             candidates are built and the one nearer to m wins, d = sqrt(sum((m - cand) * (m - cand))), the first if d1 < d2.
//
//   lanes     the same sum for n <= ALN_NP_SUM_MAX_N elements, split so that the 64 lanes of a wave (aln_pairset_transform_kernel,
//             aln_pairset.hip) can run it and the host can replay it lane by lane.  aln_np_sum_plan_make lists the leaves of the tree
//             above in order (offset, length, and how many pairs of finished subtrees close after each leaf); 24 x 24 gives eight
//             leaves of 72, other n up to ALN_NP_SUM_MAX_LEAVES uneven ones with tails.  Lane l owns running sum l % 8 of leaf
//             l / 8 (+ 8 per further round): aln_np_sum_lane_partial adds its elements in the leaf's own order (a leaf of fewer
//             than 8 elements is lane l % 8 == 0's alone, from 0.0).  aln_np_sum_combine then does per leaf the fixed
//             ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), adds its tail in turn, and closes the subtrees left + right, in
//             one thread: every addition of aln_np_sum, each with the same operands, so the same bits.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define ALN_TRANSFORM_MAX_ENTRIES 8192u
#ifndef ALN_TRANSFORM_NO_ROOT
#define ALN_TRANSFORM_NO_ROOT 1          /* status of a matrix without a real root: Err(WrongMatrixSpecified) */
#endif
// host / device qualifier of every function below: nothing for a host compiler
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ALN_RULES_HD __host__ __device__
#else
#define ALN_RULES_HD
#endif

ALN_RULES_HD inline double aln_np_pairwise(const double *a, size_t n)
{
    if (n < 8) {
        double r = 0.0;
        for (size_t i = 0; i < n; ++i) r += a[i];
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        size_t i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    size_t h = n / 2;
    h -= h % 8;
    return aln_np_pairwise(a, h) + aln_np_pairwise(a + h, n - h);
}
ALN_RULES_HD inline double aln_np_sum(const double *a, size_t n) { return 0.0 + aln_np_pairwise(a, n); }

// ---- the sum over 64 lanes
#define ALN_NP_SUM_MAX_N 1024u           /* = ALN_PAIRSET_MAX_ENTRIES */
#define ALN_NP_SUM_MAX_LEAVES 16u        /* n <= 1024: at most 16 leaves (every n is checked by the plan itself) */
#define ALN_NP_SUM_ROUNDS 2u             /* 8 leaves x 8 running sums per round of 64 lanes */
struct aln_np_sum_plan {
    uint32_t n, n_leaves;
    uint16_t off[ALN_NP_SUM_MAX_LEAVES], len[ALN_NP_SUM_MAX_LEAVES];
    uint8_t closes[ALN_NP_SUM_MAX_LEAVES];      // subtrees closed (left + right) once leaf k is done
};

// the leaves of aln_np_pairwise(a, n) from left to right; 0, or -1 for an n outside 1 .. ALN_NP_SUM_MAX_N
ALN_RULES_HD inline int aln_np_sum_plan_make(size_t n, aln_np_sum_plan *pl)
{
    pl->n = (uint32_t)n; pl->n_leaves = 0;
    if (n == 0 || n > ALN_NP_SUM_MAX_N) return -1;
    uint32_t s_off[12], s_len[12], s_depth[12], sp = 0;      // segments still to visit, the leftmost on top
    uint32_t open[12], n_open = 0;                           // depths of the finished subtrees that wait for their right sibling
    s_off[0] = 0; s_len[0] = (uint32_t)n; s_depth[0] = 0; sp = 1;
    while (sp) {
        --sp;
        const uint32_t off = s_off[sp], len = s_len[sp], depth = s_depth[sp];
        if (len > 128) {
            uint32_t h = len / 2;
            h -= h % 8;
            if (sp + 2 > 12) return -1;
            s_off[sp] = off + h; s_len[sp] = len - h; s_depth[sp] = depth + 1; ++sp;
            s_off[sp] = off; s_len[sp] = h; s_depth[sp] = depth + 1; ++sp;
            continue;
        }
        if (pl->n_leaves == ALN_NP_SUM_MAX_LEAVES) return -1;
        const uint32_t k = pl->n_leaves++;
        pl->off[k] = (uint16_t)off; pl->len[k] = (uint16_t)len;
        uint32_t d = depth, closes = 0;
        while (n_open && open[n_open - 1] == d) { --n_open; --d; ++closes; }
        if (n_open == 12) return -1;
        open[n_open++] = d;
        pl->closes[k] = (uint8_t)closes;
    }
    return 0;
}

// lane 0 .. 63, round 0 .. ALN_NP_SUM_ROUNDS - 1: running sum lane % 8 of leaf round * 8 + lane / 8 (0.0 where there is none)
ALN_RULES_HD inline double aln_np_sum_lane_partial(const aln_np_sum_plan *pl, const double *a, uint32_t lane, uint32_t round)
{
    const uint32_t k = round * 8u + (lane >> 3), j = lane & 7u;
    if (k >= pl->n_leaves) return 0.0;
    const uint32_t len = pl->len[k];
    const double *x = a + pl->off[k];
    if (len < 8) {
        double r = 0.0;
        if (j == 0) for (uint32_t i = 0; i < len; ++i) r += x[i];
        return r;
    }
    double r = x[j];
    for (uint32_t i = 8; i < len - (len % 8); i += 8) r += x[i + j];
    return r;
}

// part[round * 64 + lane] = aln_np_sum_lane_partial(pl, a, lane, round): the bits of aln_np_sum(a, pl->n)
ALN_RULES_HD inline double aln_np_sum_combine(const aln_np_sum_plan *pl, const double *a, const double *part)
{
    double st[12];
    uint32_t sp = 0;
    for (uint32_t k = 0; k < pl->n_leaves; ++k) {
        const double *r = part + (k >> 3) * 64u + (k & 7u) * 8u;
        const uint32_t len = pl->len[k];
        double v = r[0];
        if (len >= 8) {
            v = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
            for (uint32_t i = len - (len % 8); i < len; ++i) v += a[pl->off[k] + i];
        }
        st[sp++] = v;
        for (uint32_t c = pl->closes[k]; c; --c) { --sp; st[sp - 1] = st[sp - 1] + st[sp]; }
    }
    return 0.0 + st[0];
}

// returns the number of roots (0, 1, 2) of x^2 + a1 x + a0, ascending in x[]
ALN_RULES_HD inline int aln_roots_monic_quadratic(double a1, double a0, double x[2])
{
    const double a2 = 1.0;
    const double disc = a1 * a1 - (4.0 * a2) * a0;
    if (disc < 0.0) return 0;
    const double a2x2 = 2.0 * a2;
    if (disc == 0.0) { x[0] = -a1 / a2x2; return 1; }
    const double sq = sqrt(disc);
    double same, diff;
    if (a1 < 0.0) { same = -a1 + sq; diff = -a1 - sq; }
    else { same = -a1 - sq; diff = -a1 + sq; }
    double x1, x2;
    if (fabs(same) > fabs(a2x2)) {
        const double a0x2 = 2.0 * a0;
        x1 = a0x2 / same;
        x2 = fabs(diff) > fabs(a2x2) ? a0x2 / diff : same / a2x2;
    } else {
        x1 = diff / a2x2;
        x2 = same / a2x2;
    }
    if (x1 < x2) { x[0] = x1; x[1] = x2; }
    else { x[0] = x2; x[1] = x1; }
    return 2;
}

// one matrix; work: 2 * rows * cols doubles (p, base) + rows * cols of scratch.  out may not alias m.
ALN_RULES_HD inline int aln_transform_one(uint32_t rows, uint32_t cols, const double *m, const double *freq, double kd, double r_squared, double *out,
                             double *work)
{
    const size_t n = (size_t)rows * cols;
    double *p = work, *base = work + n, *tmp = work + 2 * n;
    const double f = 1.0 / (double)cols;
    for (uint32_t t = 0; t < rows; ++t)
        for (uint32_t q = 0; q < cols; ++q) p[(size_t)t * cols + q] = freq[t] * f;
    for (size_t i = 0; i < n; ++i) tmp[i] = p[i] * p[i];
    const double p2 = aln_np_sum(tmp, n);
    for (size_t i = 0; i < n; ++i) tmp[i] = p[i] * m[i];
    const double k0 = aln_np_sum(tmp, n);
    const double a = (kd - k0) / p2, b = kd / p2;
    const double amb = a - b;
    for (size_t i = 0; i < n; ++i) base[i] = m[i] + p[i] * amb;
    for (size_t i = 0; i < n; ++i) tmp[i] = base[i] * base[i];
    const double den = aln_np_sum(tmp, n);
    for (size_t i = 0; i < n; ++i) tmp[i] = p[i] * base[i];
    const double a1 = ((2.0 * b) * aln_np_sum(tmp, n)) / den;
    const double a0 = ((b * b) * p2 - r_squared) / den;
    double x[2];
    const int nr = aln_roots_monic_quadratic(a1, a0, x);
    if (nr == 0) return ALN_TRANSFORM_NO_ROOT;
    int pick = 0;
    if (nr == 2) {
        if (x[0] > 0.0 && x[1] < 0.0) pick = 0;
        else if (x[0] < 0.0 && x[1] > 0.0) pick = 1;
        else {
            double d[2];
            for (int r = 0; r < 2; ++r) {
                for (size_t i = 0; i < n; ++i) { const double c = p[i] * b + x[r] * base[i], e = m[i] - c; tmp[i] = e * e; }
                d[r] = sqrt(aln_np_sum(tmp, n));
            }
            pick = d[0] < d[1] ? 0 : 1;
        }
    }
    for (size_t i = 0; i < n; ++i) out[i] = p[i] * b + x[pick] * base[i];
    return 0;
}
