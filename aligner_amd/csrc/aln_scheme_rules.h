// aln_scheme_rules.h -- which kernel family a call's scoring scheme can run on (call_init, aln_host.hip): plain arithmetic on
// the scheme's numbers and the call's longest pair, no HIP, so that a test can compile it on a machine without a GPU.
//
// The limits, each with what it protects:
//   * integer kernels: every value integral and |H| < 2^30 for every cell, i.e. maxabs * max_span < 2^30.  Legacy
//     semantics are i32 in the reference: past this bound they have no exact form here (UNSUPPORTED); core goes to f64.
//   * dyadic schemes: a real-valued core scheme whose numbers are all multiples of 2^-k (smallest k <= 8) is filled as the
//     integer scheme times 2^k, if that scheme stays inside the integer bound.
//   * fast integer kernels: the query profile holds 4*s - 2 as int8 (aln_fast.h; sign-extended), so -31 <= s <= 32; the
//     keys 4*H + tag are i32, so maxabs * max_span < 2^28; S and four waves' profiles share the 64 KiB of LDS.
//   * matrix size: S lives in LDS -- at most 4096 entries, or 8000 for a position-weight matrix (4 x 2000, 62.5 KiB as f64).
// maxabs is the largest of |del|, |ext| and |S|; max_span the largest N + M + 2 over the call's pairs (0 without a pair).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

static constexpr uint32_t ALN_MAX_MATRIX_ENTRIES = 4096;       // substitution matrix
static constexpr uint32_t ALN_MAX_PWM_ENTRIES = 8000;          // position-weight matrix (4 x 2000)
static constexpr int ALN_MAX_DYADIC_K = 8;                     // scale factors 2^1 .. 2^8
static constexpr double ALN_INT_BOUND = 1073741824.0;          // 2^30: |H| of the integer kernels
static constexpr double ALN_FAST_BOUND = 268435456.0;          // 2^28: keys 4*H + tag of the fast kernels
static constexpr double ALN_FAST_SMIN = -31.0, ALN_FAST_SMAX = 32.0;   // int8 profile entries 4*s - 2
static constexpr uint64_t ALN_FAST_LDS = 65536;                // S + four waves' profiles

// a value the integer kernels can hold exactly
inline bool aln_integral(double v) { return isfinite(v) && v == floor(v) && fabs(v) < 1e9; }

// the matrix fits in LDS (otherwise ALN_ERR_UNSUPPORTED)
inline bool aln_matrix_fits(bool pwm, uint32_t rows, uint32_t cols)
{
    return (uint64_t)rows * cols <= (pwm ? ALN_MAX_PWM_ENTRIES : ALN_MAX_MATRIX_ENTRIES);
}

struct AlnScheme {
    bool all_int;            // del, ext (core only) and every entry integral -- after a dyadic scale, of the scaled scheme
    double maxabs, smin, smax;   // of the scheme as filled (scaled); smin <= 0 <= smax (the scan starts at 0)
    double scale;            // 2^k: the integer kernels fill the scheme times this and the scores come back times 1 / scale
    bool is_int, fast;
    uint64_t fast_lds;       // LDS bytes of S and the fast kernels' profiles
};

// The scheme's numbers: md is the matrix, compact row-major, n entries.  For the legacy semantics ext plays no part.
inline AlnScheme aln_scheme_scan(bool core, double del, double ext, const double *md, size_t n)
{
    AlnScheme s;
    s.maxabs = fabs(del) < fabs(ext) ? fabs(ext) : fabs(del);
    s.all_int = aln_integral(del) && (core ? aln_integral(ext) : true);
    s.smin = 0; s.smax = 0;
    for (size_t i = 0; i < n; ++i) {
        const double v = md[i];
        s.all_int = s.all_int && aln_integral(v);
        if (fabs(v) > s.maxabs) s.maxabs = fabs(v);
        if (v < s.smin) s.smin = v;
        if (v > s.smax) s.smax = v;
    }
    s.scale = 1.0;
    s.is_int = false; s.fast = false; s.fast_lds = 0;
    return s;
}

// Dyadic scale of a real-valued core scheme: the smallest 2^k, k <= 8, that makes every number integral -- kept only if the
// scaled scheme stays inside the integer bound (a larger k would not help: it scales maxabs further).  Core semantics only, and
// not with f64 forced, with the H output (the dump is what the kernels computed) or switched off (off: ALN_NO_DYADIC).  Updates
// s; the caller scales its own copy of the scheme by s.scale.
inline void aln_scheme_dyadic(AlnScheme &s, bool core, bool force_f64, bool want_h, bool off, double del, double ext, const double *md,
                              size_t n, uint64_t max_span)
{
    if (!core || s.all_int || force_f64 || want_h || off) return;
    for (int k = 1; k <= ALN_MAX_DYADIC_K; ++k) {
        const double sc = (double)(1 << k);
        bool ok = aln_integral(del * sc) && aln_integral(ext * sc);
        for (size_t i = 0; ok && i < n; ++i) ok = aln_integral(md[i] * sc);
        if (!ok) continue;
        if (s.maxabs * sc * (double)max_span < ALN_INT_BOUND) {
            s.maxabs *= sc; s.smin *= sc; s.smax *= sc;
            s.all_int = true;
            s.scale = sc;
        }
        return;
    }
}

// integer and fast kernels.  full_r: rows per lane of a full strip (ALN_FULL_R): a wave's profile is cols x 64 x full_r bytes.
inline void aln_scheme_route(AlnScheme &s, bool pwm, uint32_t rows, uint32_t cols, uint64_t max_span, bool force_f64, bool want_h,
                             bool force_serial, bool force_generic, uint32_t full_r)
{
    s.is_int = s.all_int && !force_f64 && s.maxabs * (double)max_span < ALN_INT_BOUND;
    s.fast_lds = (((uint64_t)rows * cols * 4 + 15) & ~15ull) + (pwm ? 0ull : 4ull * cols * 64u * full_r);
    s.fast = s.is_int && !want_h && !force_serial && !force_generic && s.fast_lds <= ALN_FAST_LDS && s.smin >= ALN_FAST_SMIN &&
             s.smax <= ALN_FAST_SMAX && s.maxabs * (double)max_span < ALN_FAST_BOUND;
}
