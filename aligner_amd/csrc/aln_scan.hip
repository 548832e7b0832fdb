// aln_scan.hip -- device side of the window scan (aln_scan_*, include/aligner_hip.h): the kernels that stand between a resident
// chromosome and the existing fill / traceback machinery of aln_kernels.hip.
//
//   expand     window k of a geometry (first, step, width, reverse) -> PairDesc k (+ queue entry k): the descriptors the batch
//              fill kernels read, built where they are used instead of on the host
//   f          the f of every window out of the 48-byte summaries (8 bytes per window go back instead of 48)
//   select     z = (f - mean) / sd >= z_min per window, compacted in ascending window order by the shared two-level prefix sum
//              (aln_select.h; a predicate and an emitter here): the same indices every run
//   hits       the selected windows -> PairDesc[cap] of the re-fill with directions (unused entries are skipped by the kernels)
//   reverse    the reversed strand, written once behind the forward one in the scan's own buffer
//   held       a held pass (aln_scan_hits) leaves every hit's summary and strings in the slot; held_f gathers the hits' f, freq sums
//              the frequency matrices (alignment.rs:55-65) of a list of held hits in unsigned integers, gather packs the listed
//              hits' summaries and strings for one download
//
// Every store is a plain C++ store or an atomicAdd of a thread (vector memory instructions).  The z test is a true IEEE division and compare
// (-ffp-contract=off, no reciprocal): NaN fails it, +inf passes it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "aln_device.h"
#include "aln_launch.h"
#include "aln_scheme_rules.h"
#include "aln_select.h"

// ---- window expansion: descriptor k = window j = first + k * step, rows seq[j .. min(j + width, len)) of the strand at `base`
__global__ __launch_bounds__(256) void aln_scan_expand_kernel(PairDesc *descs, uint32_t *order, uint64_t n, uint64_t first,
                                                              uint64_t step, uint64_t width, uint64_t len, uint64_t base,
                                                              uint32_t cols)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t j = first + k * step;
    const uint64_t rem = len - j;
    PairDesc d;
    d.q_off = 0;
    d.t_off = base + j;
    d.N = cols;
    d.M = (uint32_t)(width < rem ? width : rem);
    d.dir_off = 0; d.tb_off = 0; d.tag_off = 0; d.h_off = 0;
    d.status = ALN_OK;
    d.layout = 0;
    descs[k] = d;
    order[k] = (uint32_t)k;
}

// ---- f of every window (+ the first status that is not ALN_OK, as a flag word: the pass failed)
__global__ __launch_bounds__(256) void aln_scan_f_kernel(const aln_pair_result *res, double *f, uint64_t n, int32_t *bad)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const aln_pair_result r = res[k];
    f[k] = r.f;
    if (r.status != ALN_OK) atomicMax(bad, r.status);
}

__device__ __forceinline__ bool scan_keep(double f, double mean, double sd, double z_min)
{
    const double z = (f - mean) / sd;     // IEEE quotient (no contraction: -ffp-contract=off); a NaN z compares false
    return z >= z_min;
}

// ---- selection (aln_select.h): window k is kept by its z; kept window k goes to idx[o], the first `cap` of all
struct ScanKeep {
    const aln_pair_result *res;
    double mean, sd, z_min;
    __device__ bool operator()(uint64_t k) const { return scan_keep(res[k].f, mean, sd, z_min); }
};
struct ScanEmit {
    uint32_t *idx;
    uint32_t cap;
    __device__ void operator()(uint32_t o, uint64_t k) const { if (o < cap) idx[o] = (uint32_t)k; }
};

// ---- the re-fill's descriptors: entry h < min(count, cap) is window idx[h], laid out at h * stride in dirs / strings / tags;
// the others are skipped by every kernel (ALN_PRE_EMPTY_OK: nothing to align)
__global__ __launch_bounds__(256) void aln_scan_hits_kernel(PairDesc *descs, uint32_t *order, uint32_t n_slots, const uint32_t *idx,
                                                            const uint32_t *count, uint32_t cap, uint64_t first, uint64_t step,
                                                            uint64_t width, uint64_t len, uint64_t base, uint32_t cols,
                                                            uint64_t dir_stride, uint64_t tb_stride, uint64_t tag_stride)
{
    const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= n_slots) return;
    const uint32_t live = count[0] < cap ? count[0] : cap;
    PairDesc d;
    d.q_off = 0;
    d.N = cols;
    d.dir_off = (uint64_t)h * dir_stride; d.tb_off = (uint64_t)h * tb_stride; d.tag_off = (uint64_t)h * tag_stride; d.h_off = 0;
    d.layout = 0;
    if (h < live) {
        const uint64_t j = first + (uint64_t)idx[h] * step;
        const uint64_t rem = len - j;
        d.t_off = base + j;
        d.M = (uint32_t)(width < rem ? width : rem);
        d.status = ALN_OK;
    } else {
        d.t_off = base;
        d.M = 0;
        d.status = ALN_PRE_EMPTY_OK;
    }
    descs[h] = d;
    order[h] = h;
}

// ---- held hits: f of hit h out of its summary (the re-fill's results lie in hit order)
__global__ __launch_bounds__(256) void aln_scan_held_f_kernel(const aln_pair_result *res, double *f, uint32_t n)
{
    const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h < n) f[h] = res[h].f;
}

// ---- held hits: counts[c * cols + col - 1] += 1 for every position of every listed hit whose column number is not 0 and whose
// residue is not Blank (alignment.rs:55-65, summed over the list).  A workgroup takes a run of `per` listed hits, one wave a hit at a
// time: lane l reads positions l, l + 64, ... of the expanded strings (u32 column numbers, then the residues at 4 * (N + M + 2)),
// so both move in whole lines.  Counters are u32: LDS atomics per workgroup (within one hit a column occurs once, conflicts are
// between the waves' hits only), then one agent-scope atomicAdd per non-zero counter into the zeroed global array.  Integer sums do
// not depend on the order of arrival: the same matrix every run, and the host's.  The counters always fit: a position-weight
// matrix has at most ALN_MAX_PWM_ENTRIES = 4 x 2000 entries (aln_scheme_rules.h), 32 000 bytes of u32.
static_assert(4u * ALN_MAX_PWM_ENTRIES <= 32768u, "the frequency counters of the widest PWM must fit a workgroup's LDS");
__global__ __launch_bounds__(256) void aln_scan_freq_kernel(const PairDesc *descs, const aln_pair_result *res, const uint8_t *tb,
                                                            const uint32_t *keep, uint32_t n_keep, uint32_t per, uint32_t n_held,
                                                            uint32_t cols, uint32_t blank, uint32_t *counts)
{
    extern __shared__ uint32_t freq_lds[];
    const uint32_t cells = 4u * cols;
    for (uint32_t i = threadIdx.x; i < cells; i += blockDim.x) freq_lds[i] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const uint32_t lo = blockIdx.x * per;
    const uint32_t hi = lo + per < n_keep ? lo + per : n_keep;
    for (uint32_t k = lo + wave; k < hi; k += waves) {
        const uint32_t h = keep[k];
        if (h >= n_held) continue;                                   // checked on the host; never read beyond the held hits
        const PairDesc &d = descs[h];
        const aln_pair_result &r = res[h];
        if (r.status != ALN_OK) continue;
        const uint32_t cap = d.N + d.M + 2u;
        const uint32_t len = r.aln_len < cap ? r.aln_len : cap;
        const uint32_t *__restrict__ numbered = reinterpret_cast<const uint32_t *>(tb + d.tb_off);
        const uint8_t *__restrict__ residues = tb + d.tb_off + 4ull * cap;
        for (uint32_t j = lane; j < len; j += 64u) {
            const uint32_t col = numbered[j], c = residues[j];
            if (col == 0u || col > cols || c == blank || c >= 4u) continue;
            atomicAdd(&freq_lds[c * cols + col - 1u], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < cells; i += blockDim.x) {
        const uint32_t v = freq_lds[i];
        if (v) __hip_atomic_fetch_add(&counts[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- held hits: the u32 sums as the f64 matrix the caller gets
__global__ __launch_bounds__(256) void aln_scan_freq_f64_kernel(const uint32_t *counts, double *out, uint32_t cells)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cells) out[i] = (double)counts[i];
}

// ---- held hits: entry k of the packed output = summary and strings (one stride, as u32 words) of held hit keep[k]
__global__ __launch_bounds__(256) void aln_scan_gather_kernel(const aln_pair_result *res, const uint8_t *tb, const uint32_t *keep,
                                                              uint32_t n_held, uint64_t stride, aln_pair_result *out_res, uint8_t *out_tb)
{
    const uint32_t k = blockIdx.x, h = keep[k];
    if (h >= n_held) return;
    if (threadIdx.x == 0) out_res[k] = res[h];
    const uint32_t *__restrict__ src = reinterpret_cast<const uint32_t *>(tb + (uint64_t)h * stride);
    uint32_t *__restrict__ dst = reinterpret_cast<uint32_t *>(out_tb + (uint64_t)k * stride);
    for (uint64_t i = threadIdx.x; i < stride / 4u; i += blockDim.x) dst[i] = src[i];
}

// ---- the reversed strand: seq[len + i] = seq[len - 1 - i]
__global__ __launch_bounds__(256) void aln_scan_reverse_kernel(uint8_t *seq, uint64_t len)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < len) seq[len + i] = seq[len - 1 - i];
}

extern "C" void aln_scan_launch_expand(PairDesc *descs, uint32_t *order, uint64_t n, uint64_t first, uint64_t step, uint64_t width,
                                       uint64_t len, uint64_t base, uint32_t cols, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_scan_expand_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, descs, order, n, first, step, width, len,
                              base, cols);
}

extern "C" void aln_scan_launch_f(const aln_pair_result *res, double *f, uint64_t n, int32_t *bad, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_scan_f_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, res, f, n, bad);
}

extern "C" uint64_t aln_scan_tiles(uint64_t n) { return aln_select_tiles(n); }

extern "C" void aln_scan_launch_select(const aln_pair_result *res, uint64_t n, double mean, double sd, double z_min, uint32_t *tile_count,
                                       uint32_t *tile_off, uint32_t *count, uint32_t *idx, uint32_t cap, hipStream_t s)
{
    aln_select_launch(ScanKeep{res, mean, sd, z_min}, ScanEmit{idx, cap}, n, tile_count, tile_off, count, s);
}

extern "C" void aln_scan_launch_hits(PairDesc *descs, uint32_t *order, uint32_t n_slots, const uint32_t *idx, const uint32_t *count,
                                     uint32_t cap, uint64_t first, uint64_t step, uint64_t width, uint64_t len, uint64_t base,
                                     uint32_t cols, uint64_t dir_stride, uint64_t tb_stride, uint64_t tag_stride, hipStream_t s)
{
    if (n_slots) hipLaunchKernelGGL(aln_scan_hits_kernel, dim3(blocks_of(n_slots, 256)), dim3(256), 0, s, descs, order, n_slots, idx, count,
                                    cap, first, step, width, len, base, cols, dir_stride, tb_stride, tag_stride);
}

extern "C" void aln_scan_launch_held_f(const aln_pair_result *res, double *f, uint32_t n, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_scan_held_f_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, res, f, n);
}

// counts: 4 * cols u32, zeroed here; out: 4 * cols f64
extern "C" void aln_scan_launch_freq(const PairDesc *descs, const aln_pair_result *res, const uint8_t *tb, const uint32_t *keep,
                                     uint32_t n_keep, uint32_t n_held, uint32_t cols, uint32_t blank, uint32_t *counts, double *out,
                                     hipStream_t s)
{
    const uint32_t cells = 4u * cols;
    (void)hipMemsetAsync(counts, 0, 4ull * cells, s);
    if (n_keep) {
        // a run of >= 16 hits per workgroup (4 per wave) pays for zeroing and flushing its counters; at most 1024 workgroups
        const uint32_t grid = std::min<uint32_t>(blocks_of(n_keep, 16), 1024u);
        const uint32_t per = blocks_of(n_keep, grid);
        hipLaunchKernelGGL(aln_scan_freq_kernel, dim3(blocks_of(n_keep, per)), dim3(256), 4u * cells, s, descs, res, tb, keep, n_keep, per,
                           n_held, cols, blank, counts);
    }
    hipLaunchKernelGGL(aln_scan_freq_f64_kernel, dim3(blocks_of(cells, 256)), dim3(256), 0, s, counts, out, cells);
}

extern "C" void aln_scan_launch_gather(const aln_pair_result *res, const uint8_t *tb, const uint32_t *keep, uint32_t n_keep, uint32_t n_held,
                                       uint64_t stride, aln_pair_result *out_res, uint8_t *out_tb, hipStream_t s)
{
    if (n_keep) hipLaunchKernelGGL(aln_scan_gather_kernel, dim3(n_keep), dim3(256), 0, s, res, tb, keep, n_held, stride, out_res, out_tb);
}

extern "C" void aln_scan_launch_reverse(uint8_t *seq, uint64_t len, hipStream_t s)
{
    if (len) hipLaunchKernelGGL(aln_scan_reverse_kernel, dim3(blocks_of(len, 256)), dim3(256), 0, s, seq, len);
}
