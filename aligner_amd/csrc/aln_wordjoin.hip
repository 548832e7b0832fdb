// aln_wordjoin.hip -- device side of the sorted word index of a resident sequence set and of the join over its posting lists
// (aln_seqset_word_index / _word_join, include/aligner_hip_wordjoin.h; the rule is aln_wordjoin_rules.h).
//
//   keys       a thread per residue position: the sequence it lies in by binary search in the offsets, then the key word << 32 | seq
//              of the window that starts there, or the all-ones key where no word starts (a code >= A, the last k - 1 positions)
//   sort       rocPRIM's device radix sort, the only part not written here: the keys over the sequence's and the word's bits, a
//              chunk's pair numbers over the bits the block's pairs need.  The host owns the temporary storage
//   distinct   aln_select.h with Keep = a key that differs from the one before it, Emit = the key: the resident list E, ascending by
//              (word, seq), every (word, sequence) once
//   n(s)       one integer atomicAdd per entry of E
//   plan       a thread per entry of E whose sequence is a query of the block: the targets of its word inside the block are a piece
//              of that word's posting list, found by two binary searches on E: where it starts, how long it is, and the length added
//              to the query's 64-bit total
//   offsets    the exclusive prefix sum of the lengths of the entries whose query lies in the chunk's rows (0 for the others)
//   expand     a thread per OUTPUT position: its entry by binary search in the offsets, its target from the posting list, the pair
//              number by aln_prefilter_rank.  A word that every record carries is spread over as many threads as it has occurrences
//   classify   after the sort: the first position of a run of equal pair numbers finds the run's end by binary search; the length
//              is `shared`; aln_prefilter_candidate decides
//   append     aln_select.h with Keep = the flag, Emit = (pair number, shared)
//
// Every index is compared with the size of what it indexes, in 64 bits, before it is used; every loop is a binary search (at most 64
// trips) or runs to a count the host passed.  Every store is a plain C++ store of a thread; the atomics are integer atomicAdd.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "aln_device.h"
#include "aln_launch.h"
#include "aln_wordjoin_rules.h"
#include "aln_select.h"

constexpr uint32_t ALN_WJ_THREADS = 256u;

// the first index in [0, n) whose key is >= x (n if none): at most 64 trips
__device__ __forceinline__ uint64_t wj_lower_bound(const uint64_t *a, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    for (uint32_t trip = 0; trip < 64u && lo < hi; ++trip) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (a[mid] < x) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// ---- the key of every residue position
__global__ __launch_bounds__(256) void aln_wordjoin_keys_kernel(const uint8_t *seqs, const uint64_t *seq_off, const uint32_t *seq_len,
                                                                uint64_t n_seqs, uint64_t total, uint32_t k, uint32_t alphabet, uint64_t *keys)
{
    const uint64_t p = (uint64_t)blockIdx.x * ALN_WJ_THREADS + threadIdx.x;
    if (p >= total) return;
    // the last sequence whose offset is <= p: empty ones before it share its offset, the ones after it start beyond p
    uint64_t lo = 0, hi = n_seqs;                      // the first sequence whose offset is > p
    for (uint32_t trip = 0; trip < 64u && lo < hi; ++trip) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (seq_off[mid] <= p) lo = mid + 1u;
        else hi = mid;
    }
    uint64_t key = ALN_WORDJOIN_NO_KEY;
    if (lo >= 1u && lo <= n_seqs) {
        const uint64_t s = lo - 1u, i = p - seq_off[s];
        uint32_t w;
        if (i < seq_len[s] && i + k <= seq_len[s] && aln_prefilter_word(seqs + p, k, alphabet, &w)) key = aln_wordjoin_key(w, (uint32_t)s);
    }
    keys[p] = key;
}

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

// the targets a query q of the block meets: [*t_lo, *t_end)
__device__ __forceinline__ void wj_targets(const aln_seqset_block &b, uint64_t q, uint64_t *t_lo, uint64_t *t_end)
{
    if (b.upper) { *t_lo = q + 1u; *t_end = b.q_first + b.q_count; }
    else { *t_lo = b.t_first; *t_end = b.t_first + b.t_count; }
}

// ---- where every entry's piece of its word's posting list starts, how long it is, and the occurrences per query row
__global__ __launch_bounds__(256) void aln_wordjoin_plan_kernel(const uint64_t *entries, uint64_t n_entries, aln_seqset_block block,
                                                                uint32_t *piece_first, uint32_t *piece_len, unsigned long long *occ)
{
    const uint64_t i = (uint64_t)blockIdx.x * ALN_WJ_THREADS + threadIdx.x;
    if (i >= n_entries) return;
    const uint64_t key = entries[i];
    const uint64_t q = aln_wordjoin_key_seq(key);
    uint32_t first = 0, len = 0;
    if (q >= block.q_first && q - block.q_first < block.q_count) {
        uint64_t t_lo, t_end;
        wj_targets(block, q, &t_lo, &t_end);
        if (t_lo < t_end) {                            // (t_end <= n_seqs < 2^32: both fit a key's low half)
            const uint64_t w = key & 0xFFFFFFFF00000000ull;
            const uint64_t a = wj_lower_bound(entries, n_entries, w | t_lo), z = wj_lower_bound(entries, n_entries, w | t_end);
            if (a < z) {
                first = (uint32_t)a; len = (uint32_t)(z - a);
                atomicAdd(&occ[q - block.q_first], (unsigned long long)(z - a));
            }
        }
    }
    piece_first[i] = first;
    piece_len[i] = len;
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

// ---- output position p of the chunk -> the pair number of (its entry's query, the target at its place in the piece)
__global__ __launch_bounds__(256) void aln_wordjoin_expand_kernel(const uint64_t *entries, const uint32_t *piece_first, const uint32_t *piece_len,
                                                                  const uint32_t *offsets, uint64_t n_entries, uint64_t n_out, aln_seqset_block block,
                                                                  uint64_t pairs, uint64_t q_lo, uint64_t q_rows, uint64_t *out, uint32_t *errors)
{
    const uint64_t p = (uint64_t)blockIdx.x * ALN_WJ_THREADS + threadIdx.x;
    if (p >= n_out) return;
    uint64_t lo = 0, hi = n_entries;                   // the first entry whose offset is > p: the one before it holds p
    for (uint32_t trip = 0; trip < 64u && lo < hi; ++trip) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (offsets[mid] <= p) lo = mid + 1u;
        else hi = mid;
    }
    uint64_t number = ~0ull;
    if (lo >= 1u && lo <= n_entries) {
        const uint64_t i = lo - 1u, j = p - offsets[i];
        const uint64_t q = aln_wordjoin_key_seq(entries[i]);
        const uint64_t at = (uint64_t)piece_first[i] + j;
        if (q >= q_lo && q - q_lo < q_rows && j < piece_len[i] && at < n_entries) {
            const uint64_t t = aln_wordjoin_key_seq(entries[at]);
            uint64_t t_lo, t_end;
            wj_targets(block, q, &t_lo, &t_end);
            if ((entries[at] >> 32) == (entries[i] >> 32) && t >= t_lo && t < t_end) {
                const uint64_t r = aln_prefilter_rank(block, q, t);
                if (r < pairs) number = r;
            }
        }
    }
    if (number == ~0ull) atomicAdd(errors, 1u);         // (never on a sound index: the host turns it into ALN_ERR_DEVICE)
    out[p] = number;
}

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
        const uint64_t end = wj_lower_bound(sorted, n, number + 1u);       // (number + 1 <= pairs: no wrap)
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
    return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&aln_wordjoin_keys_kernel));
}

extern "C" int aln_wordjoin_sort_temp_bytes(uint64_t n, size_t *bytes)
{
    *bytes = 0;
    if (n == 0) return (int)hipSuccess;
    if (n > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    const uint64_t *none = nullptr;
    uint64_t *none_out = nullptr;
    return (int)rocprim::radix_sort_keys(nullptr, *bytes, none, none_out, (unsigned int)n, 0u, 64u, (hipStream_t) nullptr, false);
}

extern "C" int aln_wordjoin_launch_sort(void *temp, size_t temp_bytes, const uint64_t *in, uint64_t *out, uint64_t n, uint32_t begin_bit,
                                        uint32_t end_bit, hipStream_t s)
{
    if (n == 0) return (int)hipSuccess;
    if (n > 0x7FFFFFFFull || begin_bit >= end_bit || end_bit > 64u) return (int)hipErrorInvalidValue;
    // rocPRIM's comparison for small inputs builds its mask with a shift by end_bit, which for 64 is no shift at all unless the range
    // is the whole key: such a range must begin at bit 0
    if (end_bit == 64u && begin_bit != 0u) return (int)hipErrorInvalidValue;
    size_t need = 0;
    const hipError_t e = rocprim::radix_sort_keys(nullptr, need, in, out, (unsigned int)n, begin_bit, end_bit, s, false);
    if (e != hipSuccess) return (int)e;
    if (need > temp_bytes || (need && !temp)) return (int)hipErrorInvalidValue;
    return (int)rocprim::radix_sort_keys(temp, need, in, out, (unsigned int)n, begin_bit, end_bit, s, false);
}

extern "C" void aln_wordjoin_launch_keys(const uint8_t *seqs, const uint64_t *seq_off, const uint32_t *seq_len, uint64_t n_seqs, uint64_t total,
                                         uint32_t k, uint32_t alphabet, uint64_t *keys, hipStream_t s)
{
    if (total) hipLaunchKernelGGL(aln_wordjoin_keys_kernel, dim3(blocks_of(total, ALN_WJ_THREADS)), dim3(ALN_WJ_THREADS), 0, s, seqs, seq_off, seq_len,
                                  n_seqs, total, k, alphabet, keys);
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
    if (n_entries) hipLaunchKernelGGL(aln_wordjoin_plan_kernel, dim3(blocks_of(n_entries, ALN_WJ_THREADS)), dim3(ALN_WJ_THREADS), 0, s, entries, n_entries,
                                      *block, piece_first, piece_len, reinterpret_cast<unsigned long long *>(occ));
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
    if (n_out) hipLaunchKernelGGL(aln_wordjoin_expand_kernel, dim3(blocks_of(n_out, ALN_WJ_THREADS)), dim3(ALN_WJ_THREADS), 0, s, entries, piece_first,
                                  piece_len, offsets, n_entries, n_out, *block, pairs, q_lo, q_rows, out, errors);
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
