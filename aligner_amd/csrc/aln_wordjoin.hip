// aln_wordjoin.hip -- device side of the sorted word index of a resident sequence set and of the join over its posting lists
// (aln_seqset_word_index / _word_join, include/aligner_hip_wordjoin.h; the rule is aln_wordjoin_rules.h).
//
//   keys       aln_postings.h's, nothing kept of the position
//   sort       rocPRIM's device radix sort (aln_postings.h): the keys over the sequence's and the word's bits, a chunk's pair numbers
//              over the bits the block's pairs need.  The host owns the temporary storage
//   distinct   aln_select.h with Keep = a key that differs from the one before it, Emit = the key: the resident list E, ascending by
//              (word, seq), every (word, sequence) once
//   n(s)       one integer atomicAdd per entry of E
//   plan       aln_postings.h's over E, no entry dropped
//   offsets    the exclusive prefix sum of the lengths of the entries whose query lies in the chunk's rows (0 for the others); the
//              seed join's too
//   expand     aln_postings.h's with the pair number as the key.  A word that every record carries is spread over as many threads
//              as it has occurrences
//   classify   after the sort: the first position of a run of equal pair numbers finds the run's end by binary search; the length
//              is `shared`; aln_prefilter_candidate decides
//   append     aln_select.h with Keep = the flag, Emit = (pair number, shared)
//
// Every index is compared with the size of what it indexes, in 64 bits, before it is used; every loop is a binary search (at most 64
// trips) or runs to a count the host passed.  Every store is a plain C++ store of a thread; the atomics are integer atomicAdd.
#include "aln_postings.h"
#include "aln_launch.h"
#include "aln_select.h"

constexpr uint32_t ALN_WJ_THREADS = ALN_POSTINGS_THREADS;

struct WjDistinctKeep {
    const uint64_t *keys;
    __device__ bool operator()(uint64_t i) const { return keys[i] != ALN_WORDJOIN_NO_KEY && (i == 0 || keys[i - 1u] != keys[i]); }
};
struct WjDistinctEmit {
    const uint64_t *keys;
    uint64_t room;
    uint64_t *out;
    __device__ void operator()(uint32_t o, uint64_t i) const { if (o < room) out[o] = keys[i]; }
};

// ---- n(s): the entries of E per sequence (n_words zeroed before)
__global__ __launch_bounds__(256) void aln_wordjoin_count_kernel(const uint64_t *entries, const uint32_t *n_entries, uint64_t room, uint64_t n_seqs,
                                                                 uint32_t *n_words)
{
    const uint64_t i = (uint64_t)blockIdx.x * ALN_WJ_THREADS + threadIdx.x;
    if (i >= room || i >= n_entries[0]) return;
    const uint64_t s = aln_wordjoin_key_seq(entries[i]);
    if (s < n_seqs) atomicAdd(&n_words[s], 1u);
}

// the length that counts in a chunk of query rows q_lo .. q_lo + q_rows - 1
__device__ __forceinline__ uint32_t wj_masked(const uint64_t *entries, const uint32_t *piece_len, uint64_t i, uint64_t q_lo, uint64_t q_rows)
{
    const uint64_t q = aln_wordjoin_key_seq(entries[i]);
    return (q >= q_lo && q - q_lo < q_rows) ? piece_len[i] : 0u;
}

// ---- the masked lengths' sums per tile of aln_select.h's size, then every entry's exclusive offset (the host has bounded the total)
__global__ __launch_bounds__(256) void aln_wordjoin_tile_sums_kernel(const uint64_t *entries, const uint32_t *piece_len, uint64_t n_entries,
                                                                     uint64_t q_lo, uint64_t q_rows, uint32_t *tile_count)
{
    __shared__ uint32_t lds[ALN_SELECT_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * ALN_SELECT_TILE + (uint64_t)threadIdx.x * ALN_SELECT_PER_THREAD;
    uint32_t c = 0;
    for (uint32_t j = 0; j < ALN_SELECT_PER_THREAD; ++j)
        if (base + j < n_entries) c += wj_masked(entries, piece_len, base + j, q_lo, q_rows);
    uint32_t total;
    (void)aln_block_exclusive_scan(c, lds, &total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void aln_wordjoin_offsets_kernel(const uint64_t *entries, const uint32_t *piece_len, uint64_t n_entries,
                                                                   uint64_t q_lo, uint64_t q_rows, const uint32_t *tile_off, uint32_t *offsets)
{
    __shared__ uint32_t lds[ALN_SELECT_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * ALN_SELECT_TILE + (uint64_t)threadIdx.x * ALN_SELECT_PER_THREAD;
    uint32_t v[ALN_SELECT_PER_THREAD], c = 0;
    for (uint32_t j = 0; j < ALN_SELECT_PER_THREAD; ++j) {
        v[j] = base + j < n_entries ? wj_masked(entries, piece_len, base + j, q_lo, q_rows) : 0u;
        c += v[j];
    }
    uint32_t total;
    uint32_t o = tile_off[blockIdx.x] + aln_block_exclusive_scan(c, lds, &total);
    for (uint32_t j = 0; j < ALN_SELECT_PER_THREAD; ++j)
        if (base + j < n_entries) { offsets[base + j] = o; o += v[j]; }
}

// ---- the expansion's key: the pair number in the block
struct WjPairNumber {
    uint64_t pairs;
    __device__ bool operator()(const PostingsPair &pr, uint64_t *key) const { *key = pr.r; return pr.r < pairs; }
};

// ---- runs of equal pair numbers: shared and the keep flag at a run's first position, keep 0 elsewhere
__global__ __launch_bounds__(256) void aln_wordjoin_classify_kernel(const uint64_t *sorted, uint64_t n, aln_seqset_block block, uint64_t pairs,
                                                                    const uint32_t *n_words, uint64_t n_seqs, uint32_t min_shared,
                                                                    uint32_t min_per_1024, uint32_t *shared, uint8_t *keep)
{
    const uint64_t p = (uint64_t)blockIdx.x * ALN_WJ_THREADS + threadIdx.x;
    if (p >= n) return;
    const uint64_t number = sorted[p];
    uint32_t sh = 0;
    uint8_t kp = 0;
    if (number < pairs && (p == 0 || sorted[p - 1u] != number)) {
        const uint64_t end = aln_postings_lower_bound(sorted, n, number + 1u);       // (number + 1 <= pairs: no wrap)
        uint64_t q, t;
        aln_seqset_unrank(block, number, &q, &t);
        if (end > p && end - p <= 0xFFFFFFFFull && q < n_seqs && t < n_seqs) {
            sh = (uint32_t)(end - p);
            kp = aln_prefilter_candidate(sh, n_words[q], n_words[t], min_shared, min_per_1024) ? (uint8_t)1 : (uint8_t)0;
        }
    }
    shared[p] = sh;
    keep[p] = kp;
}

struct WjKeep {
    const uint8_t *keep;
    __device__ bool operator()(uint64_t p) const { return keep[p] != 0; }
};
struct WjEmit {
    const uint64_t *sorted;
    const uint32_t *shared;
    uint64_t room;
    uint64_t *out_k;
    uint32_t *out_shared;
    __device__ void operator()(uint32_t o, uint64_t p) const { if (o < room) { out_k[o] = sorted[p]; out_shared[o] = shared[p]; } }
};

extern "C" int aln_warm_wordjoin(void)
{
    hipFuncAttributes a;
    return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&aln_postings_keys_kernel<PostingsNoPos>));
}

extern "C" int aln_wordjoin_sort_temp_bytes(uint64_t n, size_t *bytes)
{
    return postings_sort_temp_bytes(n, bytes, [&](void *temp, size_t &size) {
        return rocprim::radix_sort_keys(temp, size, (const uint64_t *)nullptr, (uint64_t *)nullptr, (unsigned int)n, 0u, 64u, (hipStream_t) nullptr, false);
    });
}

extern "C" int aln_wordjoin_launch_sort(void *temp, size_t temp_bytes, const uint64_t *in, uint64_t *out, uint64_t n, uint32_t begin_bit,
                                        uint32_t end_bit, hipStream_t s)
{
    return postings_sort(temp, temp_bytes, n, begin_bit, end_bit, [&](void *t, size_t &size) {
        return rocprim::radix_sort_keys(t, size, in, out, (unsigned int)n, begin_bit, end_bit, s, false);
    });
}

extern "C" void aln_wordjoin_launch_keys(const uint8_t *seqs, const uint64_t *seq_off, const uint32_t *seq_len, uint64_t n_seqs, uint64_t total,
                                         uint32_t k, uint32_t alphabet, uint64_t *keys, hipStream_t s)
{
    if (total) hipLaunchKernelGGL(aln_postings_keys_kernel<PostingsNoPos>, dim3(blocks_of(total, ALN_WJ_THREADS)), dim3(ALN_WJ_THREADS), 0, s, seqs, seq_off,
                                  seq_len, n_seqs, total, k, alphabet, keys, PostingsNoPos{});
}

extern "C" void aln_wordjoin_launch_distinct(const uint64_t *sorted, uint64_t n, uint32_t *tile_count, uint32_t *tile_off, uint32_t *count,
                                             uint64_t room, uint64_t *entries, uint64_t n_seqs, uint32_t *n_words, hipStream_t s)
{
    aln_select_launch(WjDistinctKeep{sorted}, WjDistinctEmit{sorted, room, entries}, n, tile_count, tile_off, count, s);
    if (room) hipLaunchKernelGGL(aln_wordjoin_count_kernel, dim3(blocks_of(room, ALN_WJ_THREADS)), dim3(ALN_WJ_THREADS), 0, s, entries, count, room,
                                 n_seqs, n_words);
}

extern "C" void aln_wordjoin_launch_plan(const uint64_t *entries, uint64_t n_entries, const aln_seqset_block *block, uint32_t *piece_first,
                                         uint32_t *piece_len, uint64_t *occ, hipStream_t s)
{
    if (n_entries) hipLaunchKernelGGL(aln_postings_plan_kernel<PostingsDropNone>, dim3(blocks_of(n_entries, ALN_WJ_THREADS)), dim3(ALN_WJ_THREADS), 0, s,
                                      entries, n_entries, *block, PostingsDropNone{}, piece_first, piece_len, reinterpret_cast<unsigned long long *>(occ));
}

extern "C" void aln_wordjoin_launch_offsets(const uint64_t *entries, const uint32_t *piece_len, uint64_t n_entries, uint64_t q_lo, uint64_t q_rows,
                                            uint32_t *tile_count, uint32_t *tile_off, uint32_t *total, uint32_t *offsets, hipStream_t s)
{
    const uint64_t tiles = aln_select_tiles(n_entries);
    if (tiles) hipLaunchKernelGGL(aln_wordjoin_tile_sums_kernel, dim3((uint32_t)tiles), dim3(ALN_SELECT_THREADS), 0, s, entries, piece_len, n_entries, q_lo,
                                  q_rows, tile_count);
    hipLaunchKernelGGL(aln_select_offsets_kernel<uint32_t>, dim3(1), dim3(ALN_SELECT_THREADS), 0, s, tile_count, tile_off, tiles, total);
    if (tiles) hipLaunchKernelGGL(aln_wordjoin_offsets_kernel, dim3((uint32_t)tiles), dim3(ALN_SELECT_THREADS), 0, s, entries, piece_len, n_entries, q_lo,
                                  q_rows, tile_off, offsets);
}

extern "C" void aln_wordjoin_launch_expand(const uint64_t *entries, const uint32_t *piece_first, const uint32_t *piece_len, const uint32_t *offsets,
                                           uint64_t n_entries, uint64_t n_out, const aln_seqset_block *block, uint64_t pairs, uint64_t q_lo,
                                           uint64_t q_rows, uint64_t *out, uint32_t *errors, hipStream_t s)
{
    if (n_out) hipLaunchKernelGGL(aln_postings_expand_kernel<WjPairNumber>, dim3(blocks_of(n_out, ALN_WJ_THREADS)), dim3(ALN_WJ_THREADS), 0, s, entries,
                                  piece_first, piece_len, offsets, n_entries, n_out, *block, q_lo, q_rows, WjPairNumber{pairs}, out, errors);
}

extern "C" void aln_wordjoin_launch_append(const uint64_t *sorted, uint64_t n, const aln_seqset_block *block, uint64_t pairs, const uint32_t *n_words,
                                           uint64_t n_seqs, uint32_t min_shared, uint32_t min_per_1024, uint32_t *shared, uint8_t *keep,
                                           uint32_t *tile_count, uint32_t *tile_off, uint32_t *count, uint64_t room, uint64_t *out_k,
                                           uint32_t *out_shared, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_wordjoin_classify_kernel, dim3(blocks_of(n, ALN_WJ_THREADS)), dim3(ALN_WJ_THREADS), 0, s, sorted, n, *block, pairs, n_words,
                              n_seqs, min_shared, min_per_1024, shared, keep);
    aln_select_launch(WjKeep{keep}, WjEmit{sorted, shared, room, out_k, out_shared}, n, tile_count, tile_off, count, s);
}
