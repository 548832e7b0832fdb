// aln_seedjoin_rules.h -- the positional word index of a resident sequence set and the seed join over it (aln_seqset_seed_index /
// _seed_join, include/aligner_hip_seedjoin.h) as plain integer code, no HIP: the kernels (aln_seedjoin.hip), the host (aln_host.hip) and
// a CPU test driver decide with the same lines which (k, A) are taken, what a chunk's sort key is, which diagonals a band holds, which
// window of a pair wins and where the query rows of a block are cut into chunks.
//
//   parameters  word length k in 1 .. 16, alphabet size A >= 1, A^k <= 2^32 computed in uint64_t (DNA, A = 4: every k; proteins,
//               A = 20: k <= 7)
//   word        aln_prefilter_word (aln_prefilter_rules.h), as it is: a window that touches a code >= A is no word
//   occurrence  (word, seq, pos), pos the 0-based start of the window in its record: EVERY window that is a word, repeats included.
//               The index key is aln_wordjoin_key(word, seq), the value pos; the list ascends by (word, seq)
//   dropped     max_occ > 0: a word with more than max_occ occurrences in the whole resident set makes no seed; max_occ == 0: none
//   seed        (pq, pt) of a pair (q, t) of the block with the same, not dropped, word at (q, pq) and (t, pt); its diagonal is
//               d = pt - pq, which fits int32_t (positions are below 2^31)
//   band        0 .. 2^31 - 1.  c(d0), for a diagonal d0 some seed of the pair has: the seeds of the pair with d0 <= d <= d0 + band.
//               seeds(q, t) = max c(d0); diag(q, t) = the least d0 that reaches it
//   candidate   seeds >= min_seeds, min_seeds >= 1; ascending pair number of the block (aln_prefilter_rank)
//   sort key    (pair number - the chunk's first pair number) << 32 | (d + 2^31): ascending keys are ascending by (pair, diagonal)
//   chunks      aln_seedjoin_cut: aln_wordjoin_cut over the rows' seed totals, cut shorter where the run's pairs would not fit the
//               key's 32 bits (a row alone always fits: it has fewer than 2^32 pairs)
#pragma once
#include <stdint.h>

#include "aln_wordjoin_rules.h"

#define ALN_SEEDJOIN_MAX_K 16u
#define ALN_SEEDJOIN_MAX_WORDS (1ull << 32)
#define ALN_SEEDJOIN_MAX_BAND 0x7FFFFFFFu
#define ALN_SEEDJOIN_CHUNK_SEEDS (1u << 24)                // chunk_seeds == 0
#define ALN_SEEDJOIN_MAX_CHUNK_SEEDS (1u << 26)
#define ALN_SEEDJOIN_MAX_CHUNK_PAIRS (1ull << 32)          // what the key's pair field numbers

// A^k, or 0 where (k, A) is refused: k outside 1 .. 16, A == 0, A^k beyond 2^32
ALN_HD inline uint64_t aln_seedjoin_words(uint32_t k, uint32_t alphabet) { return aln_postings_words(k, alphabet, ALN_SEEDJOIN_MAX_K); }

// d + 2^31 as 32 bits: ascending in d over the whole of int32_t
ALN_HD inline uint32_t aln_seedjoin_bias(int32_t d) { return (uint32_t)d ^ 0x80000000u; }
ALN_HD inline int32_t aln_seedjoin_unbias(uint32_t biased)
{
    const uint32_t u = biased ^ 0x80000000u;
    return u < 0x80000000u ? (int32_t)u : (int32_t)(u - 0x80000000u) - 2147483647 - 1;
}

// the diagonal of a seed: positions are below 2^31, so the difference fits
ALN_HD inline int32_t aln_seedjoin_diag(uint32_t pq, uint32_t pt) { return (int32_t)((int64_t)pt - (int64_t)pq); }

ALN_HD inline uint64_t aln_seedjoin_key(uint64_t rel_pair, int32_t d) { return rel_pair << 32 | aln_seedjoin_bias(d); }
ALN_HD inline uint64_t aln_seedjoin_key_pair(uint64_t key) { return key >> 32; }
ALN_HD inline int32_t aln_seedjoin_key_diag(uint64_t key) { return aln_seedjoin_unbias((uint32_t)key); }

// the last key of the band that starts at `key`: the same pair, the diagonal d + band or the largest one there is
ALN_HD inline uint64_t aln_seedjoin_band_last(uint64_t key, uint32_t band)
{
    const uint64_t last = (key & 0xFFFFFFFFull) + band;
    return (key & 0xFFFFFFFF00000000ull) | (last > 0xFFFFFFFFull ? 0xFFFFFFFFull : last);
}

// what a window leaves in its pair's slot: more seeds win, then the earlier position (the lower d0) -- the greatest packed value.
// count >= 1, so 0 is an empty slot
ALN_HD inline uint64_t aln_seedjoin_pack(uint32_t count, uint32_t position) { return (uint64_t)count << 32 | (uint32_t)~position; }
ALN_HD inline uint32_t aln_seedjoin_packed_count(uint64_t packed) { return (uint32_t)(packed >> 32); }
ALN_HD inline uint32_t aln_seedjoin_packed_position(uint64_t packed) { return ~(uint32_t)packed; }

// One pair's seeds as n ascending keys of one pair: seeds and diag of the rule.  What the kernels compute with one thread per window
// start and an integer atomicMax per pair, as one loop (the CPU driver's; n >= 1)
ALN_HD inline void aln_seedjoin_best_window(const uint64_t *keys, uint64_t n, uint32_t band, uint64_t *seeds, int32_t *diag)
{
    uint64_t best = 0;
    for (uint64_t p = 0; p < n; ++p) {
        if (p && keys[p - 1u] == keys[p]) continue;        // a window starts where a diagonal starts
        const uint64_t c = aln_postings_upper_bound(keys, n, aln_seedjoin_band_last(keys[p], band)) - p;
        const uint64_t packed = aln_seedjoin_pack((uint32_t)c, (uint32_t)p);
        if (packed > best) best = packed;
    }
    *seeds = aln_seedjoin_packed_count(best);
    *diag = aln_seedjoin_key_diag(keys[aln_seedjoin_packed_position(best)]);
}

// pairs of query rows first .. first + n - 1 of a valid block (first + n <= q_count)
ALN_HD inline uint64_t aln_seedjoin_row_pairs(const aln_seqset_block &b, uint64_t first, uint64_t n)
{
    if (b.upper) return aln_seqset_row_start(b.q_count, first + n) - aln_seqset_row_start(b.q_count, first);
    return n * b.t_count;
}

// rows of the chunk that starts at query row `first`: aln_wordjoin_cut over the rows' seed totals, then as many of those rows as
// have at most 2^32 pairs together (a row alone has fewer: n_seqs < 2^32), found by bisection.  0 if row `first` alone is above the cap
ALN_HD inline uint64_t aln_seedjoin_cut(const uint64_t *seeds, const aln_seqset_block &b, uint64_t first, uint64_t cap)
{
    const uint64_t n = aln_wordjoin_cut(seeds, b.q_count, first, cap);
    if (n <= 1u || aln_seedjoin_row_pairs(b, first, n) <= ALN_SEEDJOIN_MAX_CHUNK_PAIRS) return n;
    uint64_t lo = 1, hi = n;                               // lo rows fit, hi rows do not
    for (uint32_t trip = 0; trip < 64u && hi - lo > 1u; ++trip) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (aln_seedjoin_row_pairs(b, first, mid) <= ALN_SEEDJOIN_MAX_CHUNK_PAIRS) lo = mid;
        else hi = mid;
    }
    return lo;
}
