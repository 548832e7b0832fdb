// aln_wordjoin_rules.h -- the sorted word index of a resident sequence set and the join over its posting lists
// (aln_seqset_word_index / _word_join, include/aligner_hip_wordjoin.h) as plain integer code, no HIP: the kernels (aln_wordjoin.hip),
// the host (aln_host.hip) and a CPU test driver decide with the same lines which (k, A) are taken, what a key is, how many bits a
// sort needs and where the query rows of a block are cut into chunks.
//
//   parameters  word length k in 1 .. 8, alphabet size A >= 1, A^k <= 2^32 computed in uint64_t (proteins, A = 20: k <= 7; DNA: every k)
//   word        aln_prefilter_word (aln_prefilter_rules.h), as it is: a word number is below A^k <= 2^32 and so are its partial sums, so
//               its 32 bits hold it.  K(s), n(s) and shared(q, t) are the prefilter's
//   key         word << 32 | seq: ascending keys are ascending by (word, seq).  A window that is no word gets ALN_WORDJOIN_NO_KEY, all
//               ones, which no word has (seq < 2^32 - 1) and which sorts last
//   candidate   aln_prefilter_candidate, as it is, with min_shared >= 1: a join sees only the pairs that share a word
//   order       aln_prefilter_rank / aln_seqset_unrank: ascending pair numbers of the block
//   bits        aln_wordjoin_bits_needed(n): the least b with 2^b >= n (0 for n <= 1): what a radix sort of numbers below n looks at
//   chunks      aln_wordjoin_cut: the longest run of whole query rows from `first` whose occurrences together stay within the cap; a row
//               without occurrences costs nothing and joins the run; a single row above the cap gives 0 rows (ALN_ERR_CAPACITY)
#pragma once
#include <stdint.h>

#include "aln_prefilter_rules.h"

#define ALN_WORDJOIN_MAX_K 8u
#define ALN_WORDJOIN_MAX_WORDS (1ull << 32)
#define ALN_WORDJOIN_CHUNK_OCCURRENCES (1u << 24)          // chunk_occurrences == 0
#define ALN_WORDJOIN_MAX_CHUNK_OCCURRENCES (1u << 26)
#define ALN_WORDJOIN_NO_KEY 0xFFFFFFFFFFFFFFFFull

// A^k, or 0 where (k, A) is refused: k outside 1 .. max_k, A == 0, A^k beyond 2^32.  Both joins' cap
ALN_HD inline uint64_t aln_postings_words(uint32_t k, uint32_t alphabet, uint32_t max_k)
{
    if (k < 1u || k > max_k || alphabet < 1u) return 0;
    uint64_t words = 1;
    for (uint32_t j = 0; j < k; ++j) {
        words *= alphabet;                                 // (below 2^32 * 2^32 before the check: the product before was <= 2^32)
        if (words > ALN_WORDJOIN_MAX_WORDS) return 0;
    }
    return words;
}
ALN_HD inline uint64_t aln_wordjoin_words(uint32_t k, uint32_t alphabet) { return aln_postings_words(k, alphabet, ALN_WORDJOIN_MAX_K); }

// the first index in [0, n) of the ascending a[] whose key is >= x (lower) or > x (upper), n if none: at most 64 trips.  Every search
// of the two joins' kernels in a sorted list (64-bit keys, 32-bit offsets) is one of these
template <class T> ALN_HD inline uint64_t aln_postings_lower_bound(const T *a, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    for (uint32_t trip = 0; trip < 64u && lo < hi; ++trip) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (a[mid] < x) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}
template <class T> ALN_HD inline uint64_t aln_postings_upper_bound(const T *a, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    for (uint32_t trip = 0; trip < 64u && lo < hi; ++trip) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (a[mid] <= x) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// the least b with 2^b >= n; 0 for n <= 1, 64 for n > 2^63
ALN_HD inline uint32_t aln_wordjoin_bits_needed(uint64_t n)
{
    uint32_t b = 0;
    while (b < 64u && ((uint64_t)1 << b) < n) ++b;
    return b;
}

ALN_HD inline uint64_t aln_wordjoin_key(uint32_t word, uint32_t seq) { return (uint64_t)word << 32 | seq; }
ALN_HD inline uint32_t aln_wordjoin_key_word(uint64_t key) { return (uint32_t)(key >> 32); }
ALN_HD inline uint32_t aln_wordjoin_key_seq(uint64_t key) { return (uint32_t)key; }

// The bits a sort of the keys of n_seqs sequences over `words` word numbers looks at: [0, *seq_end) first, then [32, *word_end), two
// passes of a radix sort that keeps equal digits in their order.  Each field gets the bits its numbers need and one more, where it
// has one: ALN_WORDJOIN_NO_KEY has that bit set and no word's key has, so it sorts behind every key in both passes.  (A full field
// needs no such bit: seq <= 2^32 - 2 is below the low half of the all-ones key.)  The zero bits between the fields are never read,
// except that a word field that reaches bit 64 is sorted as the whole key in one pass, which gives the same order
ALN_HD inline void aln_wordjoin_sort_bits(uint64_t words, uint64_t n_seqs, uint32_t *seq_end, uint32_t *word_end)
{
    const uint32_t sb = aln_wordjoin_bits_needed(n_seqs) + 1u, wb = aln_wordjoin_bits_needed(words) + 1u;
    *seq_end = sb > 32u ? 32u : sb;
    *word_end = 32u + (wb > 32u ? 32u : wb);
}

// rows of the chunk that starts at query row `first` of `rows` rows with occ[] occurrences each: as many whole rows as stay within
// `cap` together, at least one; 0 if row `first` alone is above the cap.  first < rows
ALN_HD inline uint64_t aln_wordjoin_cut(const uint64_t *occ, uint64_t rows, uint64_t first, uint64_t cap)
{
    if (occ[first] > cap) return 0;
    uint64_t sum = 0, n = 0;
    while (first + n < rows && occ[first + n] <= cap - sum) {
        sum += occ[first + n];
        ++n;
    }
    return n;
}
