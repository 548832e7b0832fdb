// aln_prefilter_rules.h -- the k-mer prefilter of a resident sequence set (aln_seqset_kmer_index / _prefilter,
// include/aligner_hip_prefilter.h) as plain integer code, no HIP: the index and sharing kernels (aln_prefilter.hip), the host
// (aln_host.hip) and a CPU test driver decide with the same lines which windows are words, where a word's bit lives and which pairs
// are candidates.
//
//   parameters  word length k in 1 .. 8, alphabet size A >= 1, A^k <= 2^18 (ALN_PREFILTER_MAX_BITS)
//   word        a window s[i .. i + k - 1] whose codes are all < A; its number is sum c_j A^(k-1-j).  A window that touches a code >= A
//               is no word.  K(s): the SET of word numbers of s, n(s) = |K(s)|; a sequence shorter than k has n = 0
//   bitmap      per sequence (A^k + 31) / 32 32-bit elements: word w is bit w & 31 of element w >> 5, the tail bits are 0.  The
//               resident table keeps a row of aln_prefilter_stride elements per sequence (a multiple of 4: rows are read 16 bytes
//               at a time), the padding 0
//   shared      |K(q) & K(t)|: the popcount of the AND of the two bitmaps
//   candidate   shared >= min_shared  and  shared * 1024 >= min_per_1024 * min(n(q), n(t)), in uint64_t; min_per_1024 in 0 .. 1024.
//               Both thresholds 0: every pair is a candidate
//   rank        the number of pair (q, t) within its block in closed form: the inverse of aln_seqset_unrank (aln_seqset_rules.h),
//               which the sharing kernel needs because its threads are (query, target) tiles, not pair numbers
#pragma once
#include <stdint.h>

#include "aln_seqset_rules.h"

#define ALN_PREFILTER_MAX_K 8u
#define ALN_PREFILTER_MAX_BITS (1u << 18)
#define ALN_PREFILTER_MAX_PER_1024 1024u
#define ALN_PREFILTER_CHUNK_PAIRS (1u << 22)

// A^k, or 0 where (k, A) is refused: k outside 1 .. 8, A == 0, A^k beyond the cap
ALN_HD inline uint32_t aln_prefilter_bits(uint32_t k, uint32_t alphabet)
{
    if (k < 1u || k > ALN_PREFILTER_MAX_K || alphabet < 1u) return 0;
    uint64_t bits = 1;
    for (uint32_t j = 0; j < k; ++j) {
        bits *= alphabet;
        if (bits > ALN_PREFILTER_MAX_BITS) return 0;
    }
    return (uint32_t)bits;
}

// elements of one bitmap, and of one row of the resident table
ALN_HD inline uint32_t aln_prefilter_elements(uint32_t bits) { return (bits + 31u) / 32u; }
ALN_HD inline uint32_t aln_prefilter_stride(uint32_t bits) { return (aln_prefilter_elements(bits) + 3u) & ~3u; }

// the window at s[0 .. k - 1]: true and its number if every code is < A
ALN_HD inline bool aln_prefilter_word(const uint8_t *s, uint32_t k, uint32_t alphabet, uint32_t *word)
{
    uint32_t w = 0;
    for (uint32_t j = 0; j < k; ++j) {
        const uint32_t c = s[j];
        if (c >= alphabet) return false;
        w = w * alphabet + c;
    }
    *word = w;
    return true;
}

// windows of a sequence of len residues
ALN_HD inline uint64_t aln_prefilter_windows(uint64_t len, uint32_t k) { return len >= k ? len - k + 1u : 0u; }

ALN_HD inline uint32_t aln_prefilter_element(uint32_t word) { return word >> 5; }
ALN_HD inline uint32_t aln_prefilter_bit(uint32_t word) { return word & 31u; }

ALN_HD inline bool aln_prefilter_candidate(uint32_t shared, uint32_t n_q, uint32_t n_t, uint32_t min_shared, uint32_t min_per_1024)
{
    const uint64_t least = n_q < n_t ? n_q : n_t;
    return shared >= min_shared && (uint64_t)shared * 1024u >= (uint64_t)min_per_1024 * least;
}

// pair (q, t) of a valid block that holds it (upper: q < t, both in the square) -> its number in the block's order
ALN_HD inline uint64_t aln_prefilter_rank(const aln_seqset_block &b, uint64_t q, uint64_t t)
{
    if (!b.upper) return (q - b.q_first) * b.t_count + (t - b.t_first);
    const uint64_t n = b.q_count, r = q - b.q_first;
    const uint64_t w = 2u * n - r - 1u;                // row r starts at r (2n - r - 1) / 2; one factor is even
    return ((r & 1u) ? r * (w / 2u) : (r / 2u) * w) + (t - q - 1u);
}
