// aln_seedjoin.hip -- device side of the positional word index of a resident sequence set and of the seed join over it
// (aln_seqset_seed_index / _seed_join, include/aligner_hip_seedjoin.h; the rule is aln_seedjoin_rules.h).
//
//   keys       aln_postings.h's, with the value beside the key: the window's position in its record
//   sort       rocPRIM's device radix sort of (key, value) pairs, the only part not written here: the sorted list P ascends by
//              (word, seq).  (The sort is stable and the threads wrote in (seq, pos) order, so the positions of one (word, seq)
//              should ascend too; nothing here relies on that -- a seed pairs an entry with EVERY entry of a piece, whatever
//              their order -- and nothing promises it.)  The host owns the temporary storage
//   count      one thread: where the all-ones keys begin in the sorted list, the occurrences of the set
//   plan       aln_postings.h's over P, with the entries of a word dropped whose run in P, found by two more binary searches, is longer
//              than max_occ; the run's first entry counts the word
//   offsets    aln_wordjoin.hip's: the exclusive prefix sum of the lengths of the entries whose query lies in the chunk's rows
//   expand     aln_postings.h's with the sort key (pair number in the chunk) << 32 | (pt - pq + 2^31); positions of 2^31 and beyond and
//              pairs outside the chunk are refused
//   windows    after the sort: every position that starts a (pair, diagonal) run finds the end of (pair, diagonal + band) by binary
//              search -- c(d0) -- and the start of its pair's run by another, and leaves count << 32 | ~position in the slot of that
//              start by an integer atomicMax: the most seeds, then the least d0
//   append     aln_select.h with Keep = a pair's first position whose slot holds min_seeds or more, Emit = (pair number, seeds, diag)
//
// Every index is compared with the size of what it indexes, in 64 bits, before it is used; every loop is a binary search (at most 64
// trips) or runs to a count the host passed.  Every store is a plain C++ store of a thread; the atomics are integer atomicAdd and
// atomicMax.
#include "aln_postings.h"
#include "aln_launch.h"
#include "aln_seedjoin_rules.h"
#include "aln_select.h"

constexpr uint32_t ALN_SJ_THREADS = ALN_POSTINGS_THREADS;

// ---- what the keys kernel keeps of a position: where its window starts in its record
struct SjPos {
    uint32_t *pos;
    __device__ void operator()(uint64_t p, uint32_t at) const { pos[p] = at; }
};

// ---- the occurrences: the sorted keys in front of the first all-ones key
__global__ void aln_seedjoin_count_kernel(const uint64_t *sorted, uint64_t n, uint32_t *count)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) count[0] = (uint32_t)aln_postings_lower_bound(sorted, n, ALN_WORDJOIN_NO_KEY);      // (n < 2^31)
}

// ---- what the plan drops: the entries of a word with more than max_occ occurrences (max_occ == 0: none); the run's first entry
// counts the word in counters[0], zeroed before
struct SjDropFrequent {
    uint32_t max_occ;
    uint32_t *counters;
    __device__ bool operator()(const uint64_t *keys, uint64_t n, uint64_t i) const
    {
        if (!max_occ) return false;
        const uint64_t w = keys[i] & ALN_POSTINGS_WORD_MASK;
        const uint64_t a = aln_postings_lower_bound(keys, n, w), z = aln_postings_upper_bound(keys, n, w | 0xFFFFFFFFull);
        const bool dropped = z > a && z - a > max_occ;
        if (dropped && a == i) atomicAdd(&counters[0], 1u);
        return dropped;
    }
};

// ---- the expansion's key: the pair's number in the chunk k_lo .. k_end - 1 and the seed's diagonal
struct SjSortKey {
    const uint32_t *pos;
    uint64_t k_lo, k_end;
    __device__ bool operator()(const PostingsPair &pr, uint64_t *key) const
    {
        if (pos[pr.i] >= 0x80000000u || pos[pr.at] >= 0x80000000u) return false;
        if (pr.r < k_lo || pr.r >= k_end || pr.r - k_lo >= ALN_SEEDJOIN_MAX_CHUNK_PAIRS) return false;
        *key = aln_seedjoin_key(pr.r - k_lo, aln_seedjoin_diag(pos[pr.i], pos[pr.at]));
        return true;
    }
};

// ---- c(d0) of every window start into its pair's slot (slots zeroed before: one per sorted position, used at a pair's first one)
__global__ __launch_bounds__(256) void aln_seedjoin_windows_kernel(const uint64_t *sorted, uint64_t n, uint64_t chunk_pairs, uint32_t band,
                                                                   unsigned long long *slots, uint32_t *errors)
{
    const uint64_t p = (uint64_t)blockIdx.x * ALN_SJ_THREADS + threadIdx.x;
    if (p >= n) return;
    const uint64_t key = sorted[p];
    if (aln_seedjoin_key_pair(key) >= chunk_pairs) { atomicAdd(errors, 1u); return; }
    if (p && sorted[p - 1u] == key) return;
    const uint64_t end = aln_postings_upper_bound(sorted, n, aln_seedjoin_band_last(key, band));
    const uint64_t start = aln_postings_lower_bound(sorted, n, key & ALN_POSTINGS_WORD_MASK);
    if (end > p && end - p <= 0xFFFFFFFFull && start <= p && p <= 0xFFFFFFFFull)
        atomicMax(&slots[start], (unsigned long long)aln_seedjoin_pack((uint32_t)(end - p), (uint32_t)p));
    else atomicAdd(errors, 1u);
}

struct SjPairStart {
    const uint64_t *sorted;
    uint64_t chunk_pairs;
    __device__ bool operator()(uint64_t p) const
    {
        const uint64_t pair = aln_seedjoin_key_pair(sorted[p]);
        return pair < chunk_pairs && (p == 0 || aln_seedjoin_key_pair(sorted[p - 1u]) != pair);
    }
};
struct SjKeep {
    SjPairStart start;
    const uint64_t *slots;
    uint32_t min_seeds;
    __device__ bool operator()(uint64_t p) const { return start(p) && aln_seedjoin_packed_count(slots[p]) >= min_seeds; }
};
struct SjEmit {
    const uint64_t *sorted, *slots;
    uint64_t n, k_lo, room;
    uint64_t *out_k;
    uint32_t *out_seeds;
    int32_t *out_diag;
    __device__ void operator()(uint32_t o, uint64_t p) const
    {
        if (o >= room) return;
        const uint64_t slot = slots[p], at = aln_seedjoin_packed_position(slot);
        out_k[o] = k_lo + aln_seedjoin_key_pair(sorted[p]);
        out_seeds[o] = aln_seedjoin_packed_count(slot);
        out_diag[o] = at < n ? aln_seedjoin_key_diag(sorted[at]) : 0;
    }
};

extern "C" int aln_warm_seedjoin(void)
{
    hipFuncAttributes a;
    return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&aln_postings_keys_kernel<SjPos>));
}

extern "C" int aln_seedjoin_sort_pairs_temp_bytes(uint64_t n, size_t *bytes)
{
    return postings_sort_temp_bytes(n, bytes, [&](void *temp, size_t &size) {
        return rocprim::radix_sort_pairs(temp, size, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                         (unsigned int)n, 0u, 64u, (hipStream_t) nullptr, false);
    });
}

extern "C" int aln_seedjoin_launch_sort_pairs(void *temp, size_t temp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *vals_in,
                                              uint32_t *vals_out, uint64_t n, uint32_t begin_bit, uint32_t end_bit, hipStream_t s)
{
    return postings_sort(temp, temp_bytes, n, begin_bit, end_bit, [&](void *t, size_t &size) {
        return rocprim::radix_sort_pairs(t, size, keys_in, keys_out, vals_in, vals_out, (unsigned int)n, begin_bit, end_bit, s, false);
    });
}

extern "C" void aln_seedjoin_launch_keys(const uint8_t *seqs, const uint64_t *seq_off, const uint32_t *seq_len, uint64_t n_seqs, uint64_t total,
                                         uint32_t k, uint32_t alphabet, uint64_t *keys, uint32_t *pos, hipStream_t s)
{
    if (total) hipLaunchKernelGGL(aln_postings_keys_kernel<SjPos>, dim3(blocks_of(total, ALN_SJ_THREADS)), dim3(ALN_SJ_THREADS), 0, s, seqs, seq_off, seq_len,
                                  n_seqs, total, k, alphabet, keys, SjPos{pos});
}

extern "C" void aln_seedjoin_launch_count(const uint64_t *sorted, uint64_t n, uint32_t *count, hipStream_t s)
{
    hipLaunchKernelGGL(aln_seedjoin_count_kernel, dim3(1), dim3(64), 0, s, sorted, n, count);
}

extern "C" void aln_seedjoin_launch_plan(const uint64_t *keys, uint64_t n, const aln_seqset_block *block, uint32_t max_occ, uint32_t *piece_first,
                                         uint32_t *piece_len, uint64_t *row_seeds, uint32_t *counters, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_postings_plan_kernel<SjDropFrequent>, dim3(blocks_of(n, ALN_SJ_THREADS)), dim3(ALN_SJ_THREADS), 0, s, keys, n, *block,
                              SjDropFrequent{max_occ, counters}, piece_first, piece_len, reinterpret_cast<unsigned long long *>(row_seeds));
}

extern "C" void aln_seedjoin_launch_expand(const uint64_t *keys, const uint32_t *pos, const uint32_t *piece_first, const uint32_t *piece_len,
                                           const uint32_t *offsets, uint64_t n, uint64_t n_out, const aln_seqset_block *block, uint64_t k_lo,
                                           uint64_t k_end, uint64_t q_lo, uint64_t q_rows, uint64_t *out, uint32_t *errors, hipStream_t s)
{
    if (n_out) hipLaunchKernelGGL(aln_postings_expand_kernel<SjSortKey>, dim3(blocks_of(n_out, ALN_SJ_THREADS)), dim3(ALN_SJ_THREADS), 0, s, keys, piece_first,
                                  piece_len, offsets, n, n_out, *block, q_lo, q_rows, SjSortKey{pos, k_lo, k_end}, out, errors);
}

extern "C" void aln_seedjoin_launch_append(const uint64_t *sorted, uint64_t n, uint64_t k_lo, uint64_t chunk_pairs, uint32_t band, uint32_t min_seeds,
                                           uint64_t *slots, uint32_t *errors, uint32_t *tile_count, uint32_t *tile_off, uint32_t *pairs_seen,
                                           uint32_t *count, uint64_t room, uint64_t *out_k, uint32_t *out_seeds, int32_t *out_diag, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_seedjoin_windows_kernel, dim3(blocks_of(n, ALN_SJ_THREADS)), dim3(ALN_SJ_THREADS), 0, s, sorted, n, chunk_pairs, band,
                              reinterpret_cast<unsigned long long *>(slots), errors);
    // the pairs with a seed: the selection's count and offsets steps alone, no list
    const SjPairStart start{sorted, chunk_pairs};
    const uint64_t tiles = aln_select_tiles(n);
    if (tiles) hipLaunchKernelGGL(aln_select_count_kernel<SjPairStart>, dim3((uint32_t)tiles), dim3(ALN_SELECT_THREADS), 0, s, start, n, tile_count);
    hipLaunchKernelGGL(aln_select_offsets_kernel<uint32_t>, dim3(1), dim3(ALN_SELECT_THREADS), 0, s, tile_count, tile_off, tiles, pairs_seen);
    aln_select_launch(SjKeep{start, slots, min_seeds}, SjEmit{sorted, slots, n, k_lo, room, out_k, out_seeds, out_diag}, n, tile_count, tile_off, count, s);
}
