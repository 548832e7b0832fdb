// aln_seedjoin.hip -- device side of the positional word index of a resident sequence set and of the seed join over it
// (aln_seqset_seed_index / _seed_join, include/aligner_hip_seedjoin.h; the rule is aln_seedjoin_rules.h).
//
//   keys       a thread per residue position: the sequence it lies in by binary search in the offsets, then the key word << 32 | seq
//              of the window that starts there (or the all-ones key where no word starts) and the value, its position in the record
//   sort       rocPRIM's device radix sort of (key, value) pairs, the only part not written here: the sorted list P ascends by
//              (word, seq).  (The sort is stable and the threads wrote in (seq, pos) order, so the positions of one (word, seq)
//              should ascend too; nothing here relies on that -- a seed pairs an entry with EVERY entry of a piece, whatever
//              their order -- and nothing promises it.)  The host owns the temporary storage
//   count      one thread: where the all-ones keys begin in the sorted list, the occurrences of the set
//   plan       a thread per entry of P: its word's run in P by two binary searches (longer than max_occ: the word is dropped, and the
//              run's first entry counts it); of an entry whose record is a query of the block, the piece of the run inside the
//              block's targets by two more: where it starts, how long it is, and the length added to the query's 64-bit total
//   offsets    aln_wordjoin.hip's: the exclusive prefix sum of the lengths of the entries whose query lies in the chunk's rows
//   expand     a thread per OUTPUT seed: its entry by binary search in the offsets, its partner from the piece, the sort key
//              (pair number in the chunk) << 32 | (pt - pq + 2^31)
//   windows    after the sort: every position that starts a (pair, diagonal) run finds the end of (pair, diagonal + band) by binary
//              search -- c(d0) -- and the start of its pair's run by another, and leaves count << 32 | ~position in the slot of that
//              start by an integer atomicMax: the most seeds, then the least d0
//   append     aln_select.h with Keep = a pair's first position whose slot holds min_seeds or more, Emit = (pair number, seeds, diag)
//
// Every index is compared with the size of what it indexes, in 64 bits, before it is used; every loop is a binary search (at most 64
// trips) or runs to a count the host passed.  Every store is a plain C++ store of a thread; the atomics are integer atomicAdd and
// atomicMax.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "aln_device.h"
#include "aln_launch.h"
#include "aln_seedjoin_rules.h"
#include "aln_select.h"

constexpr uint32_t ALN_SJ_THREADS = 256u;

// the first index in [0, n) whose key is >= x (n if none): at most 64 trips
__device__ __forceinline__ uint64_t sj_lower_bound(const uint64_t *a, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    for (uint32_t trip = 0; trip < 64u && lo < hi; ++trip) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (a[mid] < x) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// ---- the key and the position of every residue position
__global__ __launch_bounds__(256) void aln_seedjoin_keys_kernel(const uint8_t *seqs, const uint64_t *seq_off, const uint32_t *seq_len,
                                                                uint64_t n_seqs, uint64_t total, uint32_t k, uint32_t alphabet, uint64_t *keys,
                                                                uint32_t *pos)
{
    const uint64_t p = (uint64_t)blockIdx.x * ALN_SJ_THREADS + threadIdx.x;
    if (p >= total) return;
    uint64_t lo = 0, hi = n_seqs;                      // the first sequence whose offset is > p: the one before it holds p
    for (uint32_t trip = 0; trip < 64u && lo < hi; ++trip) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (seq_off[mid] <= p) lo = mid + 1u;
        else hi = mid;
    }
    uint64_t key = ALN_WORDJOIN_NO_KEY;
    uint32_t at = 0;
    if (lo >= 1u && lo <= n_seqs) {
        const uint64_t s = lo - 1u, i = p - seq_off[s];
        uint32_t w;
        if (i < seq_len[s] && i + k <= seq_len[s] && aln_prefilter_word(seqs + p, k, alphabet, &w)) {
            key = aln_wordjoin_key(w, (uint32_t)s);
            at = (uint32_t)i;
        }
    }
    keys[p] = key;
    pos[p] = at;
}

// ---- the occurrences: the sorted keys in front of the first all-ones key
__global__ void aln_seedjoin_count_kernel(const uint64_t *sorted, uint64_t n, uint32_t *count)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) count[0] = (uint32_t)sj_lower_bound(sorted, n, ALN_WORDJOIN_NO_KEY);      // (n < 2^31)
}

// the targets a query q of the block meets: [*t_lo, *t_end)
__device__ __forceinline__ void sj_targets(const aln_seqset_block &b, uint64_t q, uint64_t *t_lo, uint64_t *t_end)
{
    if (b.upper) { *t_lo = q + 1u; *t_end = b.q_first + b.q_count; }
    else { *t_lo = b.t_first; *t_end = b.t_first + b.t_count; }
}

// ---- every entry's piece of its word's run, the seeds per query row, the dropped words (counters[0], zeroed before)
__global__ __launch_bounds__(256) void aln_seedjoin_plan_kernel(const uint64_t *keys, uint64_t n, aln_seqset_block block, uint32_t max_occ,
                                                                uint32_t *piece_first, uint32_t *piece_len, unsigned long long *row_seeds,
                                                                uint32_t *counters)
{
    const uint64_t i = (uint64_t)blockIdx.x * ALN_SJ_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    const uint64_t q = aln_wordjoin_key_seq(key);
    const uint64_t w = key & 0xFFFFFFFF00000000ull;
    uint32_t first = 0, len = 0;
    bool dropped = false;
    if (max_occ) {
        const uint64_t a = sj_lower_bound(keys, n, w), z = aln_seedjoin_upper_bound(keys, n, w | 0xFFFFFFFFull);
        dropped = z > a && z - a > max_occ;
        if (dropped && a == i) atomicAdd(&counters[0], 1u);
    }
    if (!dropped && q >= block.q_first && q - block.q_first < block.q_count) {
        uint64_t t_lo, t_end;
        sj_targets(block, q, &t_lo, &t_end);
        if (t_lo < t_end) {                            // (t_end <= n_seqs < 2^32: both fit a key's low half)
            const uint64_t a = sj_lower_bound(keys, n, w | t_lo), z = sj_lower_bound(keys, n, w | t_end);
            if (a < z) {
                first = (uint32_t)a; len = (uint32_t)(z - a);
                atomicAdd(&row_seeds[q - block.q_first], (unsigned long long)(z - a));
            }
        }
    }
    piece_first[i] = first;
    piece_len[i] = len;
}

// ---- output seed p of the chunk -> its sort key
__global__ __launch_bounds__(256) void aln_seedjoin_expand_kernel(const uint64_t *keys, const uint32_t *pos, const uint32_t *piece_first,
                                                                  const uint32_t *piece_len, const uint32_t *offsets, uint64_t n, uint64_t n_out,
                                                                  aln_seqset_block block, uint64_t k_lo, uint64_t k_end, uint64_t q_lo, uint64_t q_rows,
                                                                  uint64_t *out, uint32_t *errors)
{
    const uint64_t p = (uint64_t)blockIdx.x * ALN_SJ_THREADS + threadIdx.x;
    if (p >= n_out) return;
    uint64_t lo = 0, hi = n;                           // the first entry whose offset is > p: the one before it holds p
    for (uint32_t trip = 0; trip < 64u && lo < hi; ++trip) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (offsets[mid] <= p) lo = mid + 1u;
        else hi = mid;
    }
    uint64_t key = ALN_WORDJOIN_NO_KEY;
    bool ok = false;
    if (lo >= 1u && lo <= n) {
        const uint64_t i = lo - 1u, j = p - offsets[i];
        const uint64_t q = aln_wordjoin_key_seq(keys[i]);
        const uint64_t at = (uint64_t)piece_first[i] + j;
        if (q >= q_lo && q - q_lo < q_rows && j < piece_len[i] && at < n) {
            const uint64_t t = aln_wordjoin_key_seq(keys[at]);
            uint64_t t_lo, t_end;
            sj_targets(block, q, &t_lo, &t_end);
            if ((keys[at] >> 32) == (keys[i] >> 32) && t >= t_lo && t < t_end && pos[i] < 0x80000000u && pos[at] < 0x80000000u) {
                const uint64_t r = aln_prefilter_rank(block, q, t);
                if (r >= k_lo && r < k_end && r - k_lo < ALN_SEEDJOIN_MAX_CHUNK_PAIRS) {
                    key = aln_seedjoin_key(r - k_lo, aln_seedjoin_diag(pos[i], pos[at]));
                    ok = true;
                }
            }
        }
    }
    if (!ok) atomicAdd(errors, 1u);                     // (never on a sound index: the host turns it into ALN_ERR_DEVICE)
    out[p] = key;
}

// ---- c(d0) of every window start into its pair's slot (slots zeroed before: one per sorted position, used at a pair's first one)
__global__ __launch_bounds__(256) void aln_seedjoin_windows_kernel(const uint64_t *sorted, uint64_t n, uint64_t chunk_pairs, uint32_t band,
                                                                   unsigned long long *slots, uint32_t *errors)
{
    const uint64_t p = (uint64_t)blockIdx.x * ALN_SJ_THREADS + threadIdx.x;
    if (p >= n) return;
    const uint64_t key = sorted[p];
    if (aln_seedjoin_key_pair(key) >= chunk_pairs) { atomicAdd(errors, 1u); return; }
    if (p && sorted[p - 1u] == key) return;
    const uint64_t end = aln_seedjoin_upper_bound(sorted, n, aln_seedjoin_band_last(key, band));
    const uint64_t start = sj_lower_bound(sorted, n, key & 0xFFFFFFFF00000000ull);
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
    return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&aln_seedjoin_keys_kernel));
}

extern "C" int aln_seedjoin_sort_pairs_temp_bytes(uint64_t n, size_t *bytes)
{
    *bytes = 0;
    if (n == 0) return (int)hipSuccess;
    if (n > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    const uint64_t *none = nullptr;
    uint64_t *none_out = nullptr;
    const uint32_t *vals = nullptr;
    uint32_t *vals_out = nullptr;
    return (int)rocprim::radix_sort_pairs(nullptr, *bytes, none, none_out, vals, vals_out, (unsigned int)n, 0u, 64u, (hipStream_t) nullptr, false);
}

extern "C" int aln_seedjoin_launch_sort_pairs(void *temp, size_t temp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *vals_in,
                                              uint32_t *vals_out, uint64_t n, uint32_t begin_bit, uint32_t end_bit, hipStream_t s)
{
    if (n == 0) return (int)hipSuccess;
    if (n > 0x7FFFFFFFull || begin_bit >= end_bit || end_bit > 64u) return (int)hipErrorInvalidValue;
    if (end_bit == 64u && begin_bit != 0u) return (int)hipErrorInvalidValue;       // (as aln_wordjoin_launch_sort: such a range is the whole key)
    size_t need = 0;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, need, keys_in, keys_out, vals_in, vals_out, (unsigned int)n, begin_bit, end_bit, s, false);
    if (e != hipSuccess) return (int)e;
    if (need > temp_bytes || (need && !temp)) return (int)hipErrorInvalidValue;
    return (int)rocprim::radix_sort_pairs(temp, need, keys_in, keys_out, vals_in, vals_out, (unsigned int)n, begin_bit, end_bit, s, false);
}

extern "C" void aln_seedjoin_launch_keys(const uint8_t *seqs, const uint64_t *seq_off, const uint32_t *seq_len, uint64_t n_seqs, uint64_t total,
                                         uint32_t k, uint32_t alphabet, uint64_t *keys, uint32_t *pos, hipStream_t s)
{
    if (total) hipLaunchKernelGGL(aln_seedjoin_keys_kernel, dim3(blocks_of(total, ALN_SJ_THREADS)), dim3(ALN_SJ_THREADS), 0, s, seqs, seq_off, seq_len,
                                  n_seqs, total, k, alphabet, keys, pos);
}

extern "C" void aln_seedjoin_launch_count(const uint64_t *sorted, uint64_t n, uint32_t *count, hipStream_t s)
{
    hipLaunchKernelGGL(aln_seedjoin_count_kernel, dim3(1), dim3(64), 0, s, sorted, n, count);
}

extern "C" void aln_seedjoin_launch_plan(const uint64_t *keys, uint64_t n, const aln_seqset_block *block, uint32_t max_occ, uint32_t *piece_first,
                                         uint32_t *piece_len, uint64_t *row_seeds, uint32_t *counters, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_seedjoin_plan_kernel, dim3(blocks_of(n, ALN_SJ_THREADS)), dim3(ALN_SJ_THREADS), 0, s, keys, n, *block, max_occ, piece_first,
                              piece_len, reinterpret_cast<unsigned long long *>(row_seeds), counters);
}

extern "C" void aln_seedjoin_launch_expand(const uint64_t *keys, const uint32_t *pos, const uint32_t *piece_first, const uint32_t *piece_len,
                                           const uint32_t *offsets, uint64_t n, uint64_t n_out, const aln_seqset_block *block, uint64_t k_lo,
                                           uint64_t k_end, uint64_t q_lo, uint64_t q_rows, uint64_t *out, uint32_t *errors, hipStream_t s)
{
    if (n_out) hipLaunchKernelGGL(aln_seedjoin_expand_kernel, dim3(blocks_of(n_out, ALN_SJ_THREADS)), dim3(ALN_SJ_THREADS), 0, s, keys, pos, piece_first,
                                  piece_len, offsets, n, n_out, *block, k_lo, k_end, q_lo, q_rows, out, errors);
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
