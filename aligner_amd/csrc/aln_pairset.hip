// aln_pairset.hip -- device side of the resident pair set (aln_pairset_*, include/aligner_hip.h), and the host-side batched matrix
// transform that goes with it (aln_transform_matrices).
//
//   freq      the frequency matrix (alignment.rs:13-23) of every listed pair out of its held strings: one wave per pair, lane l reads
//             columns l, l + 64, ... of both strings, counts in a u32 histogram of rows * cols bins in the wave's own LDS, and the
//             bins go out as plain stores.  Integer counts: exact, and the same whatever the order of arrival.
//   gather    the listed pairs' summaries and both strings (aln_len bytes each), packed for one download
//   transform transform_matrix for n matrices, plain C++ on the host in the order aln_transform_rules.h fixes
//
// Every store is a plain C++ store or an LDS atomicAdd of a thread (vector memory instructions).
#include <hip/hip_runtime.h>

#include <vector>

#include "aln_device.h"
#include "aln_transform_rules.h"

// ---- counts[k][t * cols + q] for listed entry k = held entry list[k]
__global__ __launch_bounds__(256) void aln_pairset_freq_kernel(const PairsetHeld *held, const aln_pair_result *res, const uint8_t *tb,
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
        const PairsetHeld d = held[h];
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

// ---- listed entry k: its summary, and both strings at out_tb + out_off[k] (query, then target cap bytes later)
__global__ __launch_bounds__(256) void aln_pairset_gather_kernel(const PairsetHeld *held, const aln_pair_result *res, const uint8_t *tb,
                                                                 const uint32_t *list, const uint64_t *out_off, uint32_t n_held,
                                                                 aln_pair_result *out_res, uint8_t *out_tb)
{
    const uint32_t k = blockIdx.x, h = list[k];
    if (h >= n_held) return;
    const aln_pair_result r = res[h];
    if (threadIdx.x == 0) out_res[k] = r;
    if (r.status != ALN_OK || !out_tb) return;
    const PairsetHeld d = held[h];
    const uint32_t cap = d.N + d.M + 2u;
    const uint32_t len = r.aln_len < cap ? r.aln_len : cap;
    const uint8_t *__restrict__ src = tb + d.tb_off;
    uint8_t *__restrict__ dst = out_tb + out_off[k];
    for (uint32_t j = threadIdx.x; j < len; j += blockDim.x) { dst[j] = src[j]; dst[cap + j] = src[cap + j]; }
}

extern "C" void aln_pairset_launch_freq(const PairsetHeld *held, const aln_pair_result *res, const uint8_t *tb, const uint32_t *list,
                                        uint32_t n_list, uint32_t n_held, uint32_t rows, uint32_t cols, uint32_t blank, uint32_t *counts,
                                        hipStream_t s)
{
    // rows * cols <= ALN_PAIRSET_MAX_ENTRIES: four waves' bins are at most 16 KiB
    if (n_list) hipLaunchKernelGGL(aln_pairset_freq_kernel, dim3((n_list + 3u) / 4u), dim3(256), 4u * 4u * rows * cols, s, held, res, tb, list,
                                   n_list, n_held, rows, cols, blank, counts);
}

extern "C" void aln_pairset_launch_gather(const PairsetHeld *held, const aln_pair_result *res, const uint8_t *tb, const uint32_t *list,
                                          const uint64_t *out_off, uint32_t n_list, uint32_t n_held, aln_pair_result *out_res, uint8_t *out_tb,
                                          hipStream_t s)
{
    if (n_list) hipLaunchKernelGGL(aln_pairset_gather_kernel, dim3(n_list), dim3(256), 0, s, held, res, tb, list, out_off, n_held, out_res, out_tb);
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
