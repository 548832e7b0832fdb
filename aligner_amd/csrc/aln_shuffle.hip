// aln_shuffle.hip -- device side of the shuffled-copy p-value batch (aln_shuffle_scores / aln_shuffle_targets,
// include/aligner_hip.h): calculate_p_value's 4 999 trimmed and shuffled copies of a target (statistics/mod.rs:240-320) are drawn
// on the device from the resident originals, and handed to the existing fill kernels as descriptors built where they are used.
//
//   shuffle   one thread per copy: its stream (aln_shuffle_rules.h), the trim, then Fisher-Yates over its own L - trim residues --
//             in a slot of LDS when the pair's target has at most ALN_SHUFFLE_LDS_MAX residues (the slot is the chunk's longest
//             such target, 64 threads per workgroup), in place in the output region otherwise.  The permutation is serial by
//             nature: a parallel sort by random keys would be a different distribution.
//   expand    copy s of pair i -> PairDesc: pair i's query, the copy's residues, M = L - trim, score only (aln_scan_expand_kernel)
//   gather    f of every copy out of the 48-byte summaries (8 bytes per copy go back), and per pair the first copy whose status
//             is not ALN_OK, as one atomicMin of (copy << 8 | status)
//
// The stream of copy s of pair i is (seed, pair_base + i, s); with a STREAM TABLE (aln_seqset_held_significance: the pairs are listed
// hits of a sequence set) it is (seed, stream[i], s) instead -- the same kernels, instantiated a second time, the pair table unchanged.
//
// Every store is a plain C++ store of a thread (vector memory instructions).
#include <hip/hip_runtime.h>

#include "aln_device.h"
#include "aln_launch.h"
#include "aln_shuffle_rules.h"

// ---- the copies of pairs p0 .. of a chunk: copy k of the chunk is copy k % per_pair of pair p0 + k / per_pair, written at
// out + (out_off - out_base) + s * t_len.  slot: LDS bytes per thread (0: no LDS; a multiple of 16, at most ALN_SHUFFLE_LDS_MAX).
// TABLE: pair i's stream index is stream[i], not pair_base + i.
template <bool TABLE>
__global__ __launch_bounds__(ALN_SHUFFLE_THREADS) void aln_shuffle_kernel(const uint8_t *seqs, uint8_t *out, const ShufflePair *pairs,
                                                                          uint32_t p0, uint64_t n, uint32_t per_pair, uint64_t seed,
                                                                          uint64_t pair_base, uint32_t max_trim, uint64_t out_base,
                                                                          uint32_t slot, const uint64_t *stream)
{
    extern __shared__ uint8_t lds[];
    const uint64_t k = (uint64_t)blockIdx.x * ALN_SHUFFLE_THREADS + threadIdx.x;
    if (k >= n) return;
    const uint32_t i = p0 + (uint32_t)(k / per_pair), s = (uint32_t)(k % per_pair);
    const ShufflePair P = pairs[i];
    uint64_t state = aln_shuffle_state(seed, TABLE ? stream[i] : pair_base + i, s);
    const uint32_t len = P.t_len - aln_shuffle_trim(state, max_trim);     // the host checked t_len >= max_trim
    const uint8_t *src = seqs + P.t_off;
    uint8_t *dst = out + (P.out_off - out_base) + (uint64_t)s * P.t_len;
    if (P.t_len <= slot) {
        uint8_t *a = lds + (uint32_t)threadIdx.x * slot;
        for (uint32_t j = 0; j < len; ++j) a[j] = src[j];
        aln_shuffle_permute(state, a, len);
        // out: bytes up to a 4-byte boundary, then dwords, then the tail
        uint32_t j = 0;
        const uint32_t head = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u);
        for (; j < head && j < len; ++j) dst[j] = a[j];
        for (; j + 4 <= len; j += 4)
            *reinterpret_cast<uint32_t *>(dst + j) = (uint32_t)a[j] | ((uint32_t)a[j + 1] << 8) | ((uint32_t)a[j + 2] << 16) | ((uint32_t)a[j + 3] << 24);
        for (; j < len; ++j) dst[j] = a[j];
    } else {
        for (uint32_t j = 0; j < len; ++j) dst[j] = src[j];
        aln_shuffle_permute(state, dst, len);
    }
}

// ---- descriptor k of a chunk = copy k: the query of its pair, the copy's residues at region + (out_off - out_base) + s * t_len
// of the residue buffer, M = L - trim (an empty query or copy: the reference panics, ALN_ERR_EMPTY_SEQUENCE as in chunk_plan)
template <bool TABLE>
__global__ __launch_bounds__(256) void aln_shuffle_expand_kernel(PairDesc *descs, uint32_t *order, const ShufflePair *pairs, uint32_t p0,
                                                                 uint64_t n, uint32_t per_pair, uint64_t seed, uint64_t pair_base,
                                                                 uint32_t max_trim, uint64_t region, uint64_t out_base, const uint64_t *stream)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t i = p0 + (uint32_t)(k / per_pair), s = (uint32_t)(k % per_pair);
    const ShufflePair P = pairs[i];
    PairDesc d;
    d.q_off = P.q_off;
    d.t_off = region + (P.out_off - out_base) + (uint64_t)s * P.t_len;
    d.N = P.q_len;
    d.M = P.t_len - aln_shuffle_trim_of(seed, TABLE ? stream[i] : pair_base + i, s, max_trim);
    d.dir_off = 0; d.tb_off = 0; d.tag_off = 0; d.h_off = 0;
    d.status = (d.N == 0 || d.M == 0) ? ALN_ERR_EMPTY_SEQUENCE : ALN_OK;
    d.layout = 0;
    descs[k] = d;
    order[k] = (uint32_t)k;
}

// ---- f of every copy of the chunk into f[k]; first[k / per_pair] = min over the failed copies of (copy << 8 | status)
__global__ __launch_bounds__(256) void aln_shuffle_gather_kernel(const aln_pair_result *res, double *f, uint64_t n, uint32_t per_pair,
                                                                 uint32_t *first)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const aln_pair_result r = res[k];
    f[k] = r.f;
    if (r.status != ALN_OK) atomicMin(first + k / per_pair, ((uint32_t)(k % per_pair) << 8) | ((uint32_t)r.status & 0xffu));
}

template <bool TABLE>
static void shuffle_launch(const uint8_t *seqs, uint8_t *out, const ShufflePair *pairs, uint32_t p0, uint64_t n, uint32_t per_pair, uint64_t seed,
                           uint64_t pair_base, uint32_t max_trim, uint64_t out_base, uint32_t slot, const uint64_t *stream, hipStream_t s)
{
    if (!n) return;
    const uint32_t lds = slot * ALN_SHUFFLE_THREADS;
    aln_launch_lds(&aln_shuffle_kernel<TABLE>, dim3(blocks_of(n, ALN_SHUFFLE_THREADS)), dim3(ALN_SHUFFLE_THREADS), lds, s, seqs, out, pairs, p0, n, per_pair,
                   seed, pair_base, max_trim, out_base, slot, stream);
}

extern "C" void aln_shuffle_launch(const uint8_t *seqs, uint8_t *out, const ShufflePair *pairs, uint32_t p0, uint64_t n, uint32_t per_pair,
                                   uint64_t seed, uint64_t pair_base, uint32_t max_trim, uint64_t out_base, uint32_t slot, hipStream_t s)
{
    shuffle_launch<false>(seqs, out, pairs, p0, n, per_pair, seed, pair_base, max_trim, out_base, slot, nullptr, s);
}

extern "C" void aln_shuffle_launch_table(const uint8_t *seqs, uint8_t *out, const ShufflePair *pairs, uint32_t p0, uint64_t n, uint32_t per_pair,
                                         uint64_t seed, const uint64_t *stream, uint32_t max_trim, uint64_t out_base, uint32_t slot, hipStream_t s)
{
    shuffle_launch<true>(seqs, out, pairs, p0, n, per_pair, seed, 0, max_trim, out_base, slot, stream, s);
}

extern "C" void aln_shuffle_launch_expand(PairDesc *descs, uint32_t *order, const ShufflePair *pairs, uint32_t p0, uint64_t n, uint32_t per_pair,
                                          uint64_t seed, uint64_t pair_base, uint32_t max_trim, uint64_t region, uint64_t out_base, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_shuffle_expand_kernel<false>, dim3(blocks_of(n, 256)), dim3(256), 0, s, descs, order, pairs, p0, n, per_pair, seed,
                              pair_base, max_trim, region, out_base, nullptr);
}

extern "C" void aln_shuffle_launch_expand_table(PairDesc *descs, uint32_t *order, const ShufflePair *pairs, uint32_t p0, uint64_t n,
                                                uint32_t per_pair, uint64_t seed, const uint64_t *stream, uint32_t max_trim, uint64_t region,
                                                uint64_t out_base, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_shuffle_expand_kernel<true>, dim3(blocks_of(n, 256)), dim3(256), 0, s, descs, order, pairs, p0, n, per_pair, seed,
                              (uint64_t)0, max_trim, region, out_base, stream);
}

extern "C" void aln_shuffle_launch_gather(const aln_pair_result *res, double *f, uint64_t n, uint32_t per_pair, uint32_t *first, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_shuffle_gather_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, res, f, n, per_pair, first);
}
