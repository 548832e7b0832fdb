// aln_postings.h -- what the word join (aln_wordjoin.hip) and the seed join (aln_seedjoin.hip) do alike on the device, each step
// once.  Both hold a list of keys word << 32 | seq ascending by (word, seq) -- a posting list per word -- and both turn a block of
// the S x S grid into the pairs that share a word by the same four steps; a route adds what its functor adds and nothing else.
//
//   keys       a thread per residue position: the sequence it lies in by binary search in the offsets, then the key of the window that
//              starts there, or the all-ones key where no word starts (a code >= A, the last k - 1 positions).  StorePos: what else a
//              route keeps of the position (the seed join: where the window starts in its record)
//   plan       a thread per entry whose sequence is a query of the block: the targets of its word inside the block are a piece of
//              that word's posting list, found by two binary searches: where it starts, how long it is, and the length added to the
//              query's 64-bit total.  Drop: the entries a route leaves out before that (the seed join: the words beyond max_occ)
//   expand     a thread per OUTPUT position of a chunk: its entry by binary search in the offsets, its partner from the piece, the
//              pair's number by aln_prefilter_rank.  MakeKey: what a route sorts the pair by, and the checks it adds
//   sort       rocPRIM's device radix sort, the only part not written here, under one statement of its argument rules
//
// Every index is compared with the size of what it indexes, in 64 bits, before it is used; every loop is a binary search (at most 64
// trips).  Every store is a plain C++ store of a thread; the atomics are integer atomicAdd.
#pragma once
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "aln_device.h"
#include "aln_wordjoin_rules.h"

constexpr uint32_t ALN_POSTINGS_THREADS = 256u;
constexpr uint64_t ALN_POSTINGS_WORD_MASK = 0xFFFFFFFF00000000ull;

// the sequence that holds residue position p: the last one whose offset is <= p -- empty ones before it share its offset, the ones
// after it start beyond p.  false if there is none
__device__ __forceinline__ bool postings_seq_of(const uint64_t *seq_off, uint64_t n_seqs, uint64_t p, uint64_t *s)
{
    const uint64_t after = aln_postings_upper_bound(seq_off, n_seqs, p);
    if (after < 1u || after > n_seqs) return false;
    *s = after - 1u;
    return true;
}

// the targets a query q of the block meets: [*t_lo, *t_end)
__device__ __forceinline__ void postings_targets(const aln_seqset_block &b, uint64_t q, uint64_t *t_lo, uint64_t *t_end)
{
    if (b.upper) { *t_lo = q + 1u; *t_end = b.q_first + b.q_count; }
    else { *t_lo = b.t_first; *t_end = b.t_first + b.t_count; }
}

// the piece [*a, *z) of the run of key's word that lies inside the targets of key's sequence as a query of the block; false if the
// sequence is no query of the block or the piece is empty
__device__ __forceinline__ bool postings_piece(const uint64_t *keys, uint64_t n, const aln_seqset_block &block, uint64_t key, uint64_t *a, uint64_t *z)
{
    const uint64_t q = aln_wordjoin_key_seq(key);
    if (q < block.q_first || q - block.q_first >= block.q_count) return false;
    uint64_t t_lo, t_end;
    postings_targets(block, q, &t_lo, &t_end);
    if (t_lo >= t_end) return false;                   // (t_end <= n_seqs < 2^32: both fit a key's low half)
    const uint64_t w = key & ALN_POSTINGS_WORD_MASK;
    *a = aln_postings_lower_bound(keys, n, w | t_lo);
    *z = aln_postings_lower_bound(keys, n, w | t_end);
    return *a < *z;
}

// output position p of a chunk of query rows q_lo .. q_lo + q_rows - 1: entry i holds it, `at` is its partner in i's piece, r the
// number of the pair (i's sequence, at's sequence) in the block.  false where p names no pair (never on a sound index)
struct PostingsPair { uint64_t i, at, r; };
__device__ __forceinline__ bool postings_walk(const uint64_t *keys, const uint32_t *piece_first, const uint32_t *piece_len, const uint32_t *offsets,
                                              uint64_t n, const aln_seqset_block &block, uint64_t q_lo, uint64_t q_rows, uint64_t p, PostingsPair *pr)
{
    const uint64_t lo = aln_postings_upper_bound(offsets, n, p);      // the first entry whose offset is > p: the one before it holds p
    if (lo < 1u || lo > n) return false;
    const uint64_t i = lo - 1u, j = p - offsets[i];
    const uint64_t q = aln_wordjoin_key_seq(keys[i]);
    const uint64_t at = (uint64_t)piece_first[i] + j;
    if (q < q_lo || q - q_lo >= q_rows || j >= piece_len[i] || at >= n) return false;
    const uint64_t t = aln_wordjoin_key_seq(keys[at]);
    uint64_t t_lo, t_end;
    postings_targets(block, q, &t_lo, &t_end);
    if ((keys[at] >> 32) != (keys[i] >> 32) || t < t_lo || t >= t_end) return false;
    pr->i = i; pr->at = at; pr->r = aln_prefilter_rank(block, q, t);
    return true;
}

// ---- the key of every residue position; store_pos(p, where the window starts in its record, 0 where no word starts)
template <class StorePos>
__global__ __launch_bounds__(256) void aln_postings_keys_kernel(const uint8_t *seqs, const uint64_t *seq_off, const uint32_t *seq_len, uint64_t n_seqs,
                                                                uint64_t total, uint32_t k, uint32_t alphabet, uint64_t *keys, StorePos store_pos)
{
    const uint64_t p = (uint64_t)blockIdx.x * ALN_POSTINGS_THREADS + threadIdx.x;
    if (p >= total) return;
    uint64_t key = ALN_WORDJOIN_NO_KEY, s;
    uint32_t at = 0;
    if (postings_seq_of(seq_off, n_seqs, p, &s)) {
        const uint64_t i = p - seq_off[s];
        uint32_t w;
        if (i < seq_len[s] && i + k <= seq_len[s] && aln_prefilter_word(seqs + p, k, alphabet, &w)) {
            key = aln_wordjoin_key(w, (uint32_t)s);
            at = (uint32_t)i;
        }
    }
    keys[p] = key;
    store_pos(p, at);
}
struct PostingsNoPos {
    __device__ void operator()(uint64_t, uint32_t) const {}
};

// ---- where every entry's piece starts, how long it is, and the total per query row (row_total zeroed before); drop(keys, n, i): the
// entries that get no piece
template <class Drop>
__global__ __launch_bounds__(256) void aln_postings_plan_kernel(const uint64_t *keys, uint64_t n, aln_seqset_block block, Drop drop, uint32_t *piece_first,
                                                                uint32_t *piece_len, unsigned long long *row_total)
{
    const uint64_t i = (uint64_t)blockIdx.x * ALN_POSTINGS_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    uint32_t first = 0, len = 0;
    uint64_t a, z;
    if (!drop(keys, n, i) && postings_piece(keys, n, block, key, &a, &z)) {
        first = (uint32_t)a; len = (uint32_t)(z - a);
        atomicAdd(&row_total[aln_wordjoin_key_seq(key) - block.q_first], (unsigned long long)(z - a));
    }
    piece_first[i] = first;
    piece_len[i] = len;
}
struct PostingsDropNone {
    __device__ bool operator()(const uint64_t *, uint64_t, uint64_t) const { return false; }
};

// ---- output position p of the chunk -> make(pair, &key), the route's sort key; the all-ones key and one more in errors[0] where the
// position names no pair or make refuses it (never on a sound index: the host turns it into ALN_ERR_DEVICE)
template <class MakeKey>
__global__ __launch_bounds__(256) void aln_postings_expand_kernel(const uint64_t *keys, const uint32_t *piece_first, const uint32_t *piece_len,
                                                                  const uint32_t *offsets, uint64_t n, uint64_t n_out, aln_seqset_block block,
                                                                  uint64_t q_lo, uint64_t q_rows, MakeKey make, uint64_t *out, uint32_t *errors)
{
    const uint64_t p = (uint64_t)blockIdx.x * ALN_POSTINGS_THREADS + threadIdx.x;
    if (p >= n_out) return;
    PostingsPair pr;
    uint64_t key = ALN_WORDJOIN_NO_KEY;
    if (!postings_walk(keys, piece_first, piece_len, offsets, n, block, q_lo, q_rows, p, &pr) || !make(pr, &key)) {
        key = ALN_WORDJOIN_NO_KEY;
        atomicAdd(errors, 1u);
    }
    out[p] = key;
}

// ---- rocPRIM's radix sort of n items over bits begin_bit .. end_bit - 1.  run(temp, bytes): the rocPRIM call, which only sizes
// `bytes` where temp is null.  n < 2^31; rocPRIM's comparison for small inputs builds its mask with a shift by end_bit, which for 64
// is no shift at all unless the range is the whole key: a range that ends at bit 64 must begin at bit 0
template <class Run> static int postings_sort_temp_bytes(uint64_t n, size_t *bytes, Run run)
{
    *bytes = 0;
    if (n == 0) return (int)hipSuccess;
    if (n > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    return (int)run(nullptr, *bytes);
}
template <class Run> static int postings_sort(void *temp, size_t temp_bytes, uint64_t n, uint32_t begin_bit, uint32_t end_bit, Run run)
{
    if (n == 0) return (int)hipSuccess;
    if (n > 0x7FFFFFFFull || begin_bit >= end_bit || end_bit > 64u) return (int)hipErrorInvalidValue;
    if (end_bit == 64u && begin_bit != 0u) return (int)hipErrorInvalidValue;
    size_t need = 0;
    const hipError_t e = run(nullptr, need);
    if (e != hipSuccess) return (int)e;
    if (need > temp_bytes || (need && !temp)) return (int)hipErrorInvalidValue;
    return (int)run(temp, need);
}
