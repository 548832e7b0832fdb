/*
 * aligner_hip_wordjoin.h -- the sorted word index of a resident sequence set: the candidate list of the k-mer prefilter made by a
 * join over posting lists instead of by ANDing the bitmaps of every pair.  A companion of aligner_hip_prefilter.h (which it
 * includes): the symbols live in the same libaligner_hip.so, under the same ALN_ABI_VERSION; the main header's list and the
 * prefilter's list of five are pinned by the project's tests, so this family brings its own header, its own mirror list
 * (_ffi.WORDJOIN_EXPORTS) and its own C99 caller (tests/abi_wordjoin.c).
 *
 * Why.  The bitmap route costs pairs x A^k / 8 bytes whatever the sequences share, and stops at A^k = 2^18.  Here every (word,
 * sequence) is sorted once; the sequences that carry a word stand side by side in the sorted list (the word's posting list), and every
 * two of them are a pair that shares that word.  Work follows what is shared, and a word number may be as large as 32 bits hold.
 *
 * The rule is the prefilter's (aligner_amd/csrc/aln_wordjoin_rules.h on top of aln_prefilter_rules.h is the rule as code):
 *   parameters  word length k in 1 .. 8, alphabet size A >= 1, A^k <= 2^32 computed in 64 bits (proteins, A = 20: k <= 7; DNA,
 *               A = 4: every k)
 *   word, K(s), n(s), shared(q, t)   exactly as in aligner_hip_prefilter.h; a word's number is held in 32 bits
 *   candidate   shared >= min_shared  and  shared * 1024 >= min_per_1024 * min(n(q), n(t)), in uint64_t arithmetic, with
 *               min_shared >= 1 and min_per_1024 in 0 .. 1024
 *   order       ascending pair number of the block, as aln_seqset_prefilter lists them; rectangles and upper blocks; the pairs
 *               (s, s) of a rectangle are listed like any other
 * Wherever both routes apply (A^k <= 2^18, min_shared >= 1) the two lists are equal, entry for entry: pair numbers, sequence numbers
 * and shared.  min_shared = 0 is refused here: a join sees only pairs that share a word.  The bitmap route with min_shared = 0 also
 * lists pairs with shared = 0 (whenever min_per_1024 = 0 or one of the two records has no word); this route never does.
 *
 * aln_seqset_word_index     builds (or replaces) the resident sorted list of the distinct (word, sequence) of the set -- 8 bytes each,
 *               ascending by word, then sequence -- and n(s) of every sequence, and drops any candidate list.  The bitmap index of
 *               aln_seqset_kmer_index, if built, stays.  n_words (optional): n(s) of every sequence, equal to what
 *               aln_seqset_kmer_index reports for the same (k, A) where both build.  ALN_ERR_OOM with nothing changed if the tables
 *               cannot be had.  A set of 2^31 residues or more: ALN_ERR_UNSUPPORTED
 * aln_seqset_word_join      replaces the candidate list with the candidates of `block`.  The result IS the prefilter's candidate
 *               state: the same resident pair numbers, the same host copy with shared and the sequence numbers, the same remembered
 *               block, the same limit of 0xFFFFFFF0 candidates (beyond: ALN_ERR_UNSUPPORTED).  aln_seqset_candidates,
 *               _candidate_scores, _candidate_hits and aln_seqset_candidate_best run on it unchanged.  spec->k / alphabet must equal
 *               the built word index.  The query rows of the block are joined in runs of whole rows of at most chunk_occurrences
 *               occurrences (an occurrence: one word of a query met in one target of the block); a single row with more is
 *               ALN_ERR_CAPACITY, decided before anything is changed: the earlier candidate list, the held hits and both indexes stay
 *
 * State.  As the prefilter's: the candidate list is separate from the held hits; word_index and word_join leave held hits untouched.
 * aln_seqset_stats: word_index and word_join put their kernels' time in ms[2], their wall time in ms[3] and what they moved in bytes[].
 *
 * Refused with ALN_ERR_INVALID_ARGUMENT, nothing written, all state intact: null pointers (n_words may be null); k or alphabet out of
 * range or A^k beyond 2^32; a spec that does not match the built word index, or no word index; min_shared == 0; min_per_1024 > 1024;
 * flags or reserved non-zero; chunk_occurrences > 2^26; an invalid block.
 */
#ifndef ALIGNER_HIP_WORDJOIN_H
#define ALIGNER_HIP_WORDJOIN_H
#include "aligner_hip_prefilter.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct aln_wordjoin_spec {
    uint32_t k, alphabet;          /* offset  0, 4: the word index the call expects: must equal the built one                   */
    uint32_t min_shared;           /* offset  8: 1 or more                                                                       */
    uint32_t min_per_1024;         /* offset 12: 0 .. 1024                                                                       */
    uint32_t chunk_occurrences;    /* offset 16: 0: 2^24; otherwise 1 .. 2^26 occurrences per run of query rows (tuning / tests) */
    uint32_t flags;                /* offset 20: 0                                                                               */
    uint64_t reserved;             /* offset 24: 0                                                                               */
} aln_wordjoin_spec;               /* 32 bytes */

int aln_seqset_word_index(aln_seqset *set, uint32_t k, uint32_t alphabet, uint32_t *n_words /* optional, n_seqs */);
int aln_seqset_word_join(aln_seqset *set, const aln_wordjoin_spec *spec, const aln_seqset_block *block, uint64_t *count);

#ifdef __cplusplus
}
#endif
#endif
