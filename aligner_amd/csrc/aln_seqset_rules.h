// aln_seqset_rules.h -- the pair order of a block of the S x S grid of a resident sequence set (aln_seqset_*, include/aligner_hip.h):
// plain integer arithmetic, no HIP, so that the host plan, the expansion kernel (aln_seqset.hip) and a CPU test driver number the
// pairs the same way.
//
//   rectangle  pair k = (q_first + k / t_count, t_first + k % t_count): the queries are the slow index
//   upper      the pairs i < j of the square first .. first + n - 1 in the order of generate_pairs (aligner-web
//              dispatcher/handlers.rs:253-264): (0,1) (0,2) .. (0,n-1) (1,2) ..; row r holds n - 1 - r pairs and starts at
//              r (2n - r - 1) / 2.  The row of a k is found by binary search on that closed form in uint64_t: a floating-point square
//              root rounds wrongly near row boundaries once n approaches 2^32.
//   sizes      n_seqs < 2^32, so a rectangle has fewer than 2^64 pairs and a triangle fewer than 2^63: every product below fits
//   chunks     aln_seqset_cut: where a pass over a block or over a candidate list is cut (host only; cells are doubles, as the
//              host's sums of them are)
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/aligner_hip.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define ALN_HD __host__ __device__
#else
#define ALN_HD
#endif

// The set's `misc` buffer: 64 32-bit counter words on the device, every call family's words in one place.  A handle's calls run one
// at a time on the set's one stream, and every user reads its words back, behind a synchronize, before its call queues anything else
// or returns; so users of the same word are never live together.  The arenas (cluster, profile, msa, cigar) carry their own counters.
//   words 0 .. 3   a pass's chunk (seqset_pass_chunks): word 0 the chunk's hit count (the threshold selection), bytes 8 .. 15 the
//                  first failed status (the gather).  Zeroed per chunk, read per chunk
//   words 8, 9     the k best: the rows' total (seqset_best_finish), 64 bits, written by the count kernel
//   the rest       the named words below; the other words are unused
#define ALN_SEQSET_MISC_WORDS 64u
// the kept count of ONE compaction: a sharing chunk of aln_seqset_prefilter, and the selection of aln_seqset_held_filter.  Written by
// the compaction's offsets step, which writes its total whatever it is (aln_select.h: for n == 0 too): no zeroing, no second word
#define ALN_SEQSET_MISC_COMPACT 16u
// the word index and the word join: ALN_SEQSET_MISC_WORD + ...  The index: KEPT holds the distinct entries (written by its compaction).
// The join zeroes the three per chunk
#define ALN_SEQSET_MISC_WORD 20u
#define ALN_SEQSET_MISC_WORD_WORDS 3u
// the seed index and the seed join: ALN_SEQSET_MISC_SEED + ...  The index: KEPT holds the occurrences (zeroed, then written by its
// count kernel).  The join zeroes the first four per chunk, and all five before the plan
#define ALN_SEQSET_MISC_SEED 24u
#define ALN_SEQSET_MISC_SEED_WORDS 5u
// the offsets of both joins' blocks (a chunk's words are read back from KEPT on: 3 for the word join, 4 for the seed join)
#define ALN_JOIN_MISC_KEPT 0u          // the pairs a chunk kept
#define ALN_JOIN_MISC_NO_PAIR 1u       // output positions that named no pair of the block
#define ALN_JOIN_MISC_SCANNED 2u       // occurrences (seeds) the chunk's offsets summed
#define ALN_JOIN_MISC_PAIRS_SEEN 3u    // seed join: the chunk's pairs with a seed
#define ALN_JOIN_MISC_DROPPED 4u       // seed join: the words max_occ dropped, counted by the plan
// the seed chains: ALN_SEQSET_MISC_CHAIN + ...  A call zeroes the four before its first launch
#define ALN_SEQSET_MISC_CHAIN 32u
#define ALN_SEQSET_MISC_CHAIN_WORDS 4u
#define ALN_CHAIN_MISC_ERRORS 0u       // what the kernels found that a sound index never shows
#define ALN_CHAIN_MISC_KEPT 1u         // the entries a filter kept (written by the compaction's offsets step)
#define ALN_CHAIN_MISC_TOTAL 2u        // words 2, 3: the chained anchors of the call, 64 bits (written by the offsets step)

// pairs of a block over a set of n_seqs sequences; 0 for an invalid block (a range past the set, upper with unequal ranges, a
// reserved word that is not 0, no pairs)
ALN_HD inline uint64_t aln_seqset_block_pairs(uint64_t n_seqs, const aln_seqset_block &b)
{
    if (b.reserved != 0u || b.upper > 1u) return 0;
    if (b.q_first > n_seqs || b.q_count > n_seqs - b.q_first) return 0;
    if (b.t_first > n_seqs || b.t_count > n_seqs - b.t_first) return 0;
    if (b.upper) {
        if (b.q_first != b.t_first || b.q_count != b.t_count) return 0;
        const uint64_t n = b.q_count;
        return (n & 1u) ? n * ((n - 1u) / 2u) : (n / 2u) * (n - 1u);
    }
    return b.q_count * b.t_count;
}

// first pair of row r of the upper triangle of an n-square, r <= n - 1 < 2^32: r (2n - r - 1) / 2 without leaving uint64_t
// (r even: r / 2 is exact; r odd: 2n - r - 1 is even)
ALN_HD inline uint64_t aln_seqset_row_start(uint64_t n, uint64_t r)
{
    const uint64_t w = 2u * n - r - 1u;
    return (r & 1u) ? r * (w / 2u) : (r / 2u) * w;
}

// pair k of a valid block, k < aln_seqset_block_pairs: absolute sequence numbers (query, target)
ALN_HD inline void aln_seqset_unrank(const aln_seqset_block &b, uint64_t k, uint64_t *q, uint64_t *t)
{
    if (!b.upper) {
        *q = b.q_first + k / b.t_count;
        *t = b.t_first + k % b.t_count;
        return;
    }
    const uint64_t n = b.q_count;
    uint64_t lo = 0, hi = n - 2u;                    // the largest row whose start is <= k
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1u) / 2u;
        if (aln_seqset_row_start(n, mid) <= k) lo = mid;
        else hi = mid - 1u;
    }
    *q = b.q_first + lo;
    *t = b.q_first + lo + 1u + (k - aln_seqset_row_start(n, lo));
}

// the inverse: the number of pair (q, t) of a valid block that holds it
ALN_HD inline uint64_t aln_seqset_rank(const aln_seqset_block &b, uint64_t q, uint64_t t)
{
    if (!b.upper) return (q - b.q_first) * b.t_count + (t - b.t_first);
    return aln_seqset_row_start(b.q_count, q - b.q_first) + (t - q - 1u);
}

// the pair after (q, t) in the block's order (the host walks a chunk's pairs with it instead of unranking each)
ALN_HD inline void aln_seqset_next(const aln_seqset_block &b, uint64_t *q, uint64_t *t)
{
    ++*t;
    if (b.upper) {
        if (*t == b.q_first + b.q_count) { ++*q; *t = *q + 1u; }
    } else if (*t == b.t_first + b.t_count) { ++*q; *t = b.t_first; }
}

// pairs first .. first + n - 1 of a valid block (first + n <= aln_seqset_block_pairs) by one unrank and n - 1 steps: q[i], t[i]
inline void aln_seqset_window(const aln_seqset_block &b, uint64_t first, uint64_t n, uint64_t *q, uint64_t *t)
{
    if (n == 0) return;
    uint64_t cq, ct;
    aln_seqset_unrank(b, first, &cq, &ct);
    for (uint64_t i = 0; i < n; ++i) {
        q[i] = cq; t[i] = ct;
        if (i + 1 < n) aln_seqset_next(b, &cq, &ct);
    }
}

// The chunks of a pass over `positions` consecutive positions (the pairs of a block in its order, or the entries of a candidate
// list) of `total` cells together: appends the chunks' position counts.  next_cells() yields the cells of the next position, first
// to last; it is not called when one chunk takes everything, so a pass that fits costs no walk.  A chunk ends where its cells reach
// `target`, unless what is left after it is a tail of under a quarter of the target, which joins it; no chunk holds more than `cap`
// positions (the queue entries are 32-bit and chunk-local).  forced: the target is a caller's order, not the set's own estimate,
// which otherwise lets everything up to 2e10 cells run as one chunk.
template <class NextCells>
inline void aln_seqset_cut(NextCells next_cells, uint64_t positions, double total, double target, bool forced, uint64_t cap,
                           std::vector<uint64_t> &counts)
{
    if (positions == 0) return;
    if (positions <= cap && (total <= 1.5 * target || (!forced && total <= 2.0e10))) { counts.push_back(positions); return; }
    uint64_t n = 0;
    double acc = 0, done = 0;
    for (uint64_t k = 0; k < positions; ++k) {
        acc += next_cells();
        ++n;
        if (n >= cap || (acc >= target && (total - done - acc >= 0.25 * target || k + 1 == positions))) {
            counts.push_back(n);
            done += acc; acc = 0; n = 0;
        }
    }
    if (n) counts.push_back(n);
}
