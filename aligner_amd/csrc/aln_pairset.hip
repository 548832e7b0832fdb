// aln_pairset.hip -- device side of the resident pair set (aln_pairset_*, include/aligner_hip.h), and the host-side batched matrix
// transform that goes with it (aln_transform_matrices).
//
//   freq      the frequency matrix (alignment.rs:13-23) of every listed pair out of its held strings: one wave per pair, lane l reads
//             columns l, l + 64, ... of both strings, counts in a u32 histogram of rows * cols bins in the wave's own LDS, and the
//             bins go out as plain stores.  Integer counts: exact, and the same whatever the order of arrival.
//   gather    the listed entries' summaries and both strings (aln_len bytes each) out of a held store, packed for one download: the
//             fetch of a pair set's held run and of a sequence set's held hits alike (held_fetch_strings, aln_host.hip)
//   transform transform_matrix for n matrices, plain C++ on the host in the order aln_transform_rules.h fixes (aln_transform_matrices), and
//             the same on the device (aln_pairset_transform_kernel): one wave per matrix, source, base and a product scratch in the
//             wave's own LDS, the element-wise passes strided over the lanes, every reduction through the lane form of the rules'
//             sum (64 partial sums into LDS, then the fixed combine, which every lane runs for itself), the quadratic and the choice
//             of the root from the rules' scalar code.  p[t][q] = freq[t] * (1.0 / cols) is one rounded product and is recomputed.
//             Only + - * / sqrt on f64, uncontracted (-ffp-contract=off): the bits of the host's.
//   pick      the listed entries of the resident matrix store, copied into the compact array a run's fill reads
//
// Every store is a plain C++ store or an LDS atomicAdd of a thread (vector memory instructions).
#include <hip/hip_runtime.h>

#include <vector>

#include "aln_device.h"
#include "aln_launch.h"
#include "aln_transform_rules.h"

// ---- counts[k][t * cols + q] for listed entry k = held entry list[k]
__global__ __launch_bounds__(256) void aln_pairset_freq_kernel(const HeldEntry *held, const aln_pair_result *res, const uint8_t *tb,
                                                               const uint32_t *list, uint32_t n_list, uint32_t n_held, uint32_t rows,
                                                               uint32_t cols, uint32_t blank, uint32_t *counts)
{
    extern __shared__ uint32_t pairset_lds[];
    const uint32_t cells = rows * cols;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t k = blockIdx.x * (blockDim.x >> 6) + wave;
    if (k >= n_list) return;                                         // whole waves leave; no workgroup barrier below
    uint32_t *bins = pairset_lds + wave * cells;
    for (uint32_t i = lane; i < cells; i += 64u) bins[i] = 0u;
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    const uint32_t h = list[k];
    if (h < n_held) {                                                // checked on the host; never read beyond the held entries
        const HeldEntry d = held[h];
        const aln_pair_result &r = res[h];
        if (r.status == ALN_OK) {
            const uint32_t cap = d.N + d.M + 2u;
            const uint32_t len = r.aln_len < cap ? r.aln_len : cap;
            const uint8_t *__restrict__ qa = tb + d.tb_off, *__restrict__ ta = tb + d.tb_off + cap;
            for (uint32_t j = lane; j < len; j += 64u) {
                const uint32_t q = qa[j], t = ta[j];
                if (q == blank || t == blank || q >= cols || t >= rows) continue;
                atomicAdd(&bins[t * cols + q], 1u);
            }
        }
    }
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    uint32_t *out = counts + (uint64_t)k * cells;
    for (uint32_t i = lane; i < cells; i += 64u) out[i] = bins[i];
}

// ---- listed entry k of a held store (a pair set's or a sequence set's): its summary, and both strings at out_tb + out_off[k] (query,
// then target cap bytes later)
__global__ __launch_bounds__(256) void aln_held_gather_kernel(const HeldEntry *held, const aln_pair_result *res, const uint8_t *tb,
                                                              const uint32_t *list, const uint64_t *out_off, uint32_t n_held,
                                                              aln_pair_result *out_res, uint8_t *out_tb)
{
    const uint32_t k = blockIdx.x, h = list[k];
    if (h >= n_held) return;                                         // checked on the host; never read beyond the held entries
    const aln_pair_result r = res[h];
    if (threadIdx.x == 0) out_res[k] = r;
    if (r.status != ALN_OK || !out_tb) return;
    const HeldEntry d = held[h];
    const uint32_t cap = d.N + d.M + 2u;
    const uint32_t len = r.aln_len < cap ? r.aln_len : cap;
    const uint8_t *__restrict__ src = tb + d.tb_off;
    uint8_t *__restrict__ dst = out_tb + out_off[k];
    for (uint32_t j = threadIdx.x; j < len; j += blockDim.x) { dst[j] = src[j]; dst[cap + j] = src[cap + j]; }
}

extern "C" void aln_pairset_launch_freq(const HeldEntry *held, const aln_pair_result *res, const uint8_t *tb, const uint32_t *list,
                                        uint32_t n_list, uint32_t n_held, uint32_t rows, uint32_t cols, uint32_t blank, uint32_t *counts,
                                        hipStream_t s)
{
    // rows * cols <= ALN_PAIRSET_MAX_ENTRIES: four waves' bins are at most 16 KiB
    if (n_list) hipLaunchKernelGGL(aln_pairset_freq_kernel, dim3((n_list + 3u) / 4u), dim3(256), 4u * 4u * rows * cols, s, held, res, tb, list,
                                   n_list, n_held, rows, cols, blank, counts);
}

extern "C" void aln_held_launch_gather(const HeldEntry *held, const aln_pair_result *res, const uint8_t *tb, const uint32_t *list,
                                       const uint64_t *out_off, uint32_t n_list, uint32_t n_held, aln_pair_result *out_res, uint8_t *out_tb,
                                       hipStream_t s)
{
    if (n_list) hipLaunchKernelGGL(aln_held_gather_kernel, dim3(n_list), dim3(256), 0, s, held, res, tb, list, out_off, n_held, out_res, out_tb);
}

// ---- transform_matrix on the device: listed entry k by wave k
__device__ __forceinline__ void pairset_wave_sync()
{
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
}

// doubles of LDS per wave: m, base, tmp, the 2 x 64 partial sums and the plan
__host__ __device__ inline uint32_t pairset_transform_wave_doubles(uint32_t n)
{
    return 3u * n + 64u * ALN_NP_SUM_ROUNDS + (uint32_t)((sizeof(aln_np_sum_plan) + 7u) / 8u);
}

// aln_np_sum(tmp, n) by the whole wave; tmp is complete in the writing lanes' program order, and free again afterwards
__device__ inline double pairset_wave_sum(const aln_np_sum_plan *pl, const double *tmp, double *part, uint32_t lane)
{
    pairset_wave_sync();
    for (uint32_t r = 0; r < ALN_NP_SUM_ROUNDS && r * 8u < pl->n_leaves; ++r) part[r * 64u + lane] = aln_np_sum_lane_partial(pl, tmp, lane, r);
    pairset_wave_sync();
    const double s = aln_np_sum_combine(pl, tmp, part);
    pairset_wave_sync();
    return s;
}

// element i = lane, lane + 64, ... of the matrix with its row t and column q kept in step (no division per element)
#define PAIRSET_EACH(i, t)                                                                                       \
    for (uint32_t i = lane, t = t0, q_ = q0; i < n; i += 64u, t += dt, q_ += dq, t += (q_ >= cols ? 1u : 0u), q_ -= (q_ >= cols ? cols : 0u))

__global__ __launch_bounds__(256) void aln_pairset_transform_kernel(const PairsetTransformArgs a, const aln_np_sum_plan plan)
{
    extern __shared__ double pairset_transform_lds[];
    const uint32_t rows = a.rows, cols = a.cols, n = rows * cols;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t k = blockIdx.x * (blockDim.x >> 6) + wave;
    if (k >= a.n_list) return;                                       // whole waves leave; no workgroup barrier below
    double *m = pairset_transform_lds + (size_t)wave * pairset_transform_wave_doubles(n), *base = m + n, *tmp = base + n, *part = tmp + n;
    aln_np_sum_plan *pl = reinterpret_cast<aln_np_sum_plan *>(part + 64u * ALN_NP_SUM_ROUNDS);
    for (uint32_t i = lane; i < sizeof(aln_np_sum_plan) / 4u; i += 64u)
        reinterpret_cast<uint32_t *>(pl)[i] = reinterpret_cast<const uint32_t *>(&plan)[i];
    const uint32_t t0 = lane / cols, q0 = lane % cols, dt = 64u / cols, dq = 64u % cols;

    // the source matrix
    if (a.shared) {
        for (uint32_t i = lane; i < n; i += 64u) m[i] = a.shared[i];
    } else if (a.own) {
        const double *src = a.own + (uint64_t)k * n;
        for (uint32_t i = lane; i < n; i += 64u) m[i] = src[i];
    } else {                                                         // the counts of aln_pairset_freq_kernel; u32 -> f64 is exact
        uint32_t *bins = reinterpret_cast<uint32_t *>(tmp);
        for (uint32_t i = lane; i < n; i += 64u) bins[i] = 0u;
        pairset_wave_sync();
        const uint32_t h = a.entry[k];
        if (h < a.n_held) {                                          // checked on the host; never read beyond the held entries
            const HeldEntry d = a.held[h];
            const aln_pair_result &r = a.res[h];
            if (r.status == ALN_OK) {
                const uint32_t cap = d.N + d.M + 2u;
                const uint32_t len = r.aln_len < cap ? r.aln_len : cap;
                const uint8_t *__restrict__ qa = a.tb + d.tb_off, *__restrict__ ta = a.tb + d.tb_off + cap;
                for (uint32_t j = lane; j < len; j += 64u) {
                    const uint32_t q = qa[j], t = ta[j];
                    if (q == a.blank || t == a.blank || q >= cols || t >= rows) continue;
                    atomicAdd(&bins[t * cols + q], 1u);
                }
            }
        }
        pairset_wave_sync();
        for (uint32_t i = lane; i < n; i += 64u) m[i] = (double)bins[i];
    }
    pairset_wave_sync();

    const uint32_t par = a.par ? a.par[k] : k;
    const double *__restrict__ freq = a.freq + (uint64_t)par * rows;
    const double kd = a.kd[par], r_squared = a.r2[par];
    const double f = 1.0 / (double)cols;

    // aln_transform_one, its statements in its order
    PAIRSET_EACH(i, t) { const double p = freq[t] * f; tmp[i] = p * p; }
    const double p2 = pairset_wave_sum(pl, tmp, part, lane);
    PAIRSET_EACH(i, t) { const double p = freq[t] * f; tmp[i] = p * m[i]; }
    const double k0 = pairset_wave_sum(pl, tmp, part, lane);
    const double ca = (kd - k0) / p2, b = kd / p2;
    const double amb = ca - b;
    PAIRSET_EACH(i, t) { const double p = freq[t] * f; const double v = m[i] + p * amb; base[i] = v; tmp[i] = v * v; }
    const double den = pairset_wave_sum(pl, tmp, part, lane);
    PAIRSET_EACH(i, t) { const double p = freq[t] * f; tmp[i] = p * base[i]; }
    const double a1 = ((2.0 * b) * pairset_wave_sum(pl, tmp, part, lane)) / den;
    const double a0 = ((b * b) * p2 - r_squared) / den;
    double x[2] = {0.0, 0.0};
    const int nr = aln_roots_monic_quadratic(a1, a0, x);
    if (nr == 0) {                                                   // the destination stays as it was
        if (lane == 0) a.status[k] = ALN_TRANSFORM_NO_ROOT;
        return;
    }
    double root = x[0];
    if (nr == 2) {
        if (x[0] > 0.0 && x[1] < 0.0) root = x[0];
        else if (x[0] < 0.0 && x[1] > 0.0) root = x[1];
        else {
            double d[2];
            for (int r = 0; r < 2; ++r) {
                const double xr = r ? x[1] : x[0];
                PAIRSET_EACH(i, t) { const double p = freq[t] * f; const double c = p * b + xr * base[i], e = m[i] - c; tmp[i] = e * e; }
                d[r] = sqrt(pairset_wave_sum(pl, tmp, part, lane));
            }
            root = d[0] < d[1] ? x[0] : x[1];
        }
    }
    double *out = a.dst + (uint64_t)(a.dst_index ? a.dst_index[k] : k) * n;
    PAIRSET_EACH(i, t) { const double p = freq[t] * f; out[i] = p * b + root * base[i]; }
    if (lane == 0) a.status[k] = 0;
}
#undef PAIRSET_EACH

// 0, or -1 for a shape the lane form of the sum does not cover (rows * cols outside 1 .. ALN_NP_SUM_MAX_N)
extern "C" int aln_pairset_launch_transform(const PairsetTransformArgs *a, hipStream_t s)
{
    aln_np_sum_plan plan;
    if (a->rows == 0 || a->cols == 0 || (uint64_t)a->rows * a->cols > ALN_NP_SUM_MAX_N || aln_np_sum_plan_make((size_t)a->rows * a->cols, &plan) != 0)
        return -1;
    if (!a->n_list) return 0;
    // 1024 entries: 25 KiB per wave.  As many waves (1 .. 4) as fit into 64 KiB, so that two or three workgroups share a CU's LDS
    const uint32_t per_wave = 8u * pairset_transform_wave_doubles(a->rows * a->cols);
    uint32_t waves = 65536u / per_wave;
    waves = waves > 4u ? 4u : waves;
    hipLaunchKernelGGL(aln_pairset_transform_kernel, dim3((a->n_list + waves - 1u) / waves), dim3(64u * waves), waves * per_wave, s, *a, plan);
    return 0;
}

// ---- out[k] = store[list[k]], matrices of e doubles
__global__ __launch_bounds__(256) void aln_pairset_pick_kernel(const double *__restrict__ store, const uint32_t *__restrict__ list, uint32_t e,
                                                               double *__restrict__ out)
{
    const double *src = store + (uint64_t)list[blockIdx.x] * e;
    double *dst = out + (uint64_t)blockIdx.x * e;
    for (uint32_t i = threadIdx.x; i < e; i += blockDim.x) dst[i] = src[i];
}

extern "C" void aln_pairset_launch_pick(const double *store, const uint32_t *list, uint32_t n_list, uint32_t e, double *out, hipStream_t s)
{
    if (n_list) hipLaunchKernelGGL(aln_pairset_pick_kernel, dim3(n_list), dim3(256), 0, s, store, list, e, out);
}

// ---- transform_matrix for n matrices (host only)
extern "C" int aln_transform_matrices(size_t n, uint32_t rows, uint32_t cols, const double *matrices_in, const double *frequencies,
                                      const double *kd, const double *r_squared, double *matrices_out, int32_t *status)
{
    if (n == 0) return ALN_OK;
    if (!matrices_in || !frequencies || !kd || !r_squared || !matrices_out || !status || rows == 0 || cols == 0 ||
        (uint64_t)rows * cols > ALN_TRANSFORM_MAX_ENTRIES)
        return ALN_ERR_INVALID_ARGUMENT;
    const size_t e = (size_t)rows * cols;
    std::vector<double> work(4 * e);
    for (size_t i = 0; i < n; ++i) {
        // (in place is allowed: the result is built in the work area first)
        double *res = work.data() + 3 * e;
        status[i] = aln_transform_one(rows, cols, matrices_in + i * e, frequencies + i * rows, kd[i], r_squared[i], res, work.data());
        if (status[i] == 0) for (size_t j = 0; j < e; ++j) matrices_out[i * e + j] = res[j];
    }
    return ALN_OK;
}
