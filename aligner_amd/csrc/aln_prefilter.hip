// aln_prefilter.hip -- device side of the k-mer prefilter of a resident sequence set (aln_seqset_kmer_index / _prefilter /
// _candidate_*, include/aligner_hip_prefilter.h; the rule is aln_prefilter_rules.h).
//
//   index      one workgroup per sequence: the bitmap of its words is built in LDS (atomicOr of a thread per window, at most 32 KiB),
//              then written as one row of the resident table, its popcount summed into n_words.  Sequences and windows are loops
//   share      the hot path.  A workgroup takes ALN_PF_QT queries x ALN_PF_TT targets, a lane one target.  The queries' rows are
//              staged in LDS, ALN_PF_ES elements of each at a time; every lane streams its own target row with 16-byte loads, and
//              each 16 bytes meet all staged queries: the query operand is read from LDS at an address the whole wave shares
//              (broadcast, no bank conflict), one AND and one accumulating popcount per element per pair.  A target element fetched
//              once serves ALN_PF_QT pairs.  The lane then writes shared and the keep flag of its pairs at their pair number within
//              the chunk (aln_prefilter_rank): a chunk is a range of pair numbers, as the chunks of a pass are
//   compact    aln_select.h with Keep = the flag, Emit = (block pair number, shared): ascending, no atomic append
//   expand     the sibling of aln_seqset_expand_kernel whose pair numbers come from a resident list
//
// Every store is a plain C++ store of a thread (vector memory instructions); the only atomics are the LDS atomicOr of the index.
#include <hip/hip_runtime.h>

#include "aln_device.h"
#include "aln_launch.h"
#include "aln_prefilter_rules.h"
#include "aln_select.h"

constexpr uint32_t ALN_PF_THREADS = 256u;
constexpr uint32_t ALN_PF_QT = 16u;                    // queries of a tile
constexpr uint32_t ALN_PF_TT = ALN_PF_THREADS;         // targets of a tile: one per lane
constexpr uint32_t ALN_PF_ES4 = 128u;                  // 16-byte pieces of a query row staged at a time: 16 x 128 x 16 = 32 KiB
constexpr uint32_t ALN_PF_INDEX_GRID = 1u << 16;       // workgroups of the index kernel at most

// ---- the bitmap and the word count of every sequence
__global__ __launch_bounds__(256) void aln_prefilter_index_kernel(const uint8_t *seqs, const uint64_t *seq_off, const uint32_t *seq_len,
                                                                  uint64_t n_seqs, uint32_t k, uint32_t alphabet, uint32_t elements,
                                                                  uint32_t stride, uint32_t *table, uint32_t *n_words)
{
    extern __shared__ uint32_t bitmap[];               // `elements` words
    __shared__ uint32_t sums[ALN_PF_THREADS];
    for (uint64_t s = blockIdx.x; s < n_seqs; s += gridDim.x) {
        for (uint32_t e = threadIdx.x; e < elements; e += ALN_PF_THREADS) bitmap[e] = 0u;
        __syncthreads();
        const uint8_t *res = seqs + seq_off[s];
        const uint64_t windows = aln_prefilter_windows(seq_len[s], k);
        for (uint64_t i = threadIdx.x; i < windows; i += ALN_PF_THREADS) {
            uint32_t w;
            if (aln_prefilter_word(res + i, k, alphabet, &w)) atomicOr(&bitmap[aln_prefilter_element(w)], 1u << aln_prefilter_bit(w));
        }
        __syncthreads();
        uint32_t *row = table + s * stride;
        uint32_t c = 0;
        for (uint32_t e = threadIdx.x; e < stride; e += ALN_PF_THREADS) {
            const uint32_t v = e < elements ? bitmap[e] : 0u;
            row[e] = v;
            c += (uint32_t)__popc(v);
        }
        uint32_t total;
        (void)aln_block_exclusive_scan(c, sums, &total);      // (ends with a barrier: the bitmap may be zeroed again)
        if (threadIdx.x == 0) n_words[s] = total;
    }
}

// ---- shared words and the keep flag of the pairs of one tile
__global__ __launch_bounds__(256) void aln_prefilter_share_kernel(const uint32_t *table, const uint32_t *n_words, uint32_t stride,
                                                                  aln_seqset_block block, uint64_t k0, uint64_t n, uint64_t q_lo,
                                                                  uint64_t q_rows, uint64_t t_lo, uint64_t t_count, uint32_t t_tiles,
                                                                  uint32_t min_shared, uint32_t min_per_1024, uint32_t *shared,
                                                                  uint8_t *keep)
{
    __shared__ uint4 qtile[ALN_PF_QT][ALN_PF_ES4];
    const uint64_t q0 = q_lo + (uint64_t)(blockIdx.x / t_tiles) * ALN_PF_QT;
    const uint64_t t0 = t_lo + (uint64_t)(blockIdx.x % t_tiles) * ALN_PF_TT;
    const uint64_t q_end = q_lo + q_rows, t_end = t_lo + t_count;
    const uint32_t nq = (uint32_t)(q_end - q0 < ALN_PF_QT ? q_end - q0 : ALN_PF_QT);
    if (block.upper && t0 + ALN_PF_TT - 1u <= q0) return;         // (the whole workgroup: no pair of this tile has q < t)
    const uint64_t t = t0 + threadIdx.x;
    const bool t_ok = t < t_end;
    const uint32_t s4 = stride / 4u;
    const uint4 *t_row = reinterpret_cast<const uint4 *>(table + (t_ok ? t : t_lo) * stride);
    uint32_t acc[ALN_PF_QT];
#pragma unroll
    for (uint32_t j = 0; j < ALN_PF_QT; ++j) acc[j] = 0u;
    for (uint32_t e0 = 0; e0 < s4; e0 += ALN_PF_ES4) {
        const uint32_t ne = s4 - e0 < ALN_PF_ES4 ? s4 - e0 : ALN_PF_ES4;
        if (e0) __syncthreads();                                  // the slice before has been read
        for (uint32_t i = threadIdx.x; i < ALN_PF_QT * ALN_PF_ES4; i += ALN_PF_THREADS) {
            const uint32_t j = i / ALN_PF_ES4, e = i % ALN_PF_ES4;
            if (e < ne) qtile[j][e] = j < nq ? reinterpret_cast<const uint4 *>(table + (q0 + j) * stride)[e0 + e] : make_uint4(0u, 0u, 0u, 0u);
        }
        __syncthreads();
        if (t_ok)
            for (uint32_t e = 0; e < ne; ++e) {
                const uint4 tv = t_row[e0 + e];
#pragma unroll
                for (uint32_t j = 0; j < ALN_PF_QT; ++j) {
                    const uint4 qv = qtile[j][e];
                    acc[j] += (uint32_t)__popc(tv.x & qv.x) + (uint32_t)__popc(tv.y & qv.y) + (uint32_t)__popc(tv.z & qv.z) +
                              (uint32_t)__popc(tv.w & qv.w);
                }
            }
    }
    if (!t_ok) return;
    const uint32_t n_t = n_words[t];
#pragma unroll
    for (uint32_t j = 0; j < ALN_PF_QT; ++j) {
        const uint64_t q = q0 + j;
        if (j >= nq || (block.upper && t <= q)) continue;
        const uint64_t kk = aln_prefilter_rank(block, q, t);
        if (kk < k0 || kk - k0 >= n) continue;                    // a pair of the rows' ends that belongs to another chunk
        shared[kk - k0] = acc[j];
        keep[kk - k0] = aln_prefilter_candidate(acc[j], n_words[q], n_t, min_shared, min_per_1024) ? (uint8_t)1 : (uint8_t)0;
    }
}

struct PrefilterKeep {
    const uint8_t *keep;
    __device__ bool operator()(uint64_t k) const { return keep[k] != 0; }
};
struct PrefilterEmit {
    const uint32_t *shared;
    uint64_t room, k0;
    uint64_t *out_k;
    uint32_t *out_shared;
    __device__ void operator()(uint32_t o, uint64_t k) const { if (o < room) { out_k[o] = k0 + k; out_shared[o] = shared[k]; } }
};

// ---- descriptor i of the chunk = pair list[i] of the block
__global__ __launch_bounds__(256) void aln_prefilter_expand_list_kernel(PairDesc *descs, uint32_t *order, uint64_t n, const uint64_t *list,
                                                                        aln_seqset_block block, const uint64_t *seq_off,
                                                                        const uint32_t *seq_len)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t q, t;
    aln_seqset_unrank(block, list[i], &q, &t);
    PairDesc d;
    d.q_off = seq_off[q];
    d.t_off = seq_off[t];
    d.N = seq_len[q];
    d.M = seq_len[t];
    d.dir_off = 0; d.tb_off = 0; d.tag_off = 0; d.h_off = 0;
    d.status = (d.N == 0 || d.M == 0) ? ALN_ERR_EMPTY_SEQUENCE : ALN_OK;
    d.layout = 0;
    descs[i] = d;
    order[i] = (uint32_t)i;
}

extern "C" void aln_prefilter_launch_index(const uint8_t *seqs, const uint64_t *seq_off, const uint32_t *seq_len, uint64_t n_seqs, uint32_t k,
                                           uint32_t alphabet, uint32_t elements, uint32_t stride, uint32_t *table, uint32_t *n_words,
                                           hipStream_t s)
{
    if (!n_seqs) return;
    const uint32_t grid = (uint32_t)(n_seqs < ALN_PF_INDEX_GRID ? n_seqs : ALN_PF_INDEX_GRID);
    hipLaunchKernelGGL(aln_prefilter_index_kernel, dim3(grid), dim3(ALN_PF_THREADS), 4u * elements, s, seqs, seq_off, seq_len, n_seqs, k, alphabet,
                       elements, stride, table, n_words);
}

extern "C" uint32_t aln_prefilter_share_blocks(uint64_t q_rows, uint64_t t_count)
{
    const uint64_t qt = (q_rows + ALN_PF_QT - 1) / ALN_PF_QT, tt = (t_count + ALN_PF_TT - 1) / ALN_PF_TT;
    if (qt == 0 || tt == 0 || tt > 0x7FFFFFFFull || qt > 0x7FFFFFFFull / tt) return 0;
    return (uint32_t)(qt * tt);
}

extern "C" void aln_prefilter_launch_share(const uint32_t *table, const uint32_t *n_words, uint32_t stride, const aln_seqset_block *block,
                                           uint64_t k0, uint64_t n, uint64_t q_lo, uint64_t q_rows, uint64_t t_lo, uint64_t t_count,
                                           uint32_t min_shared, uint32_t min_per_1024, uint32_t *shared, uint8_t *keep, hipStream_t s)
{
    const uint32_t blocks = aln_prefilter_share_blocks(q_rows, t_count);
    if (!n || !blocks) return;
    const uint32_t t_tiles = (uint32_t)((t_count + ALN_PF_TT - 1) / ALN_PF_TT);
    hipLaunchKernelGGL(aln_prefilter_share_kernel, dim3(blocks), dim3(ALN_PF_THREADS), 0, s, table, n_words, stride, *block, k0, n, q_lo, q_rows,
                       t_lo, t_count, t_tiles, min_shared, min_per_1024, shared, keep);
}

extern "C" void aln_prefilter_launch_compact(const uint8_t *keep, const uint32_t *shared, uint64_t n, uint64_t k0, uint32_t *tile_count,
                                             uint32_t *tile_off, uint32_t *count, uint64_t room, uint64_t *out_k, uint32_t *out_shared,
                                             hipStream_t s)
{
    aln_select_launch(PrefilterKeep{keep}, PrefilterEmit{shared, room, k0, out_k, out_shared}, n, tile_count, tile_off, count, s);
}

extern "C" void aln_prefilter_launch_expand_list(PairDesc *descs, uint32_t *order, uint64_t n, const uint64_t *list,
                                                 const aln_seqset_block *block, const uint64_t *seq_off, const uint32_t *seq_len, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_prefilter_expand_list_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, descs, order, n, list, *block, seq_off, seq_len);
}
