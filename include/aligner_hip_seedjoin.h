/*
 * aligner_hip_seedjoin.h -- the seed join of a resident sequence set: the candidate list of the k-mer prefilter made from word hits
 * that lie on a common diagonal.  A companion of aligner_hip_wordjoin.h (which it includes): the symbols live in the same
 * libaligner_hip.so, under the same ALN_ABI_VERSION; the other headers' lists are pinned by the project's tests, so this family brings
 * its own header, its own mirror list (_ffi.SEEDJOIN_EXPORTS) and its own C99 caller (tests/abi_seedjoin.c).
 *
 * Why.  The bitmaps and the word join count the distinct words two records share and keep no positions: two records that carry copies
 * of one repeat, or that share a few words scattered anywhere, pass like a true overlap.  A true overlap puts its word hits on one
 * diagonal (target position - query position roughly constant); chance and repeats scatter them.  Here every occurrence of a word
 * keeps its position, a pair is judged by the most seeds it has within one band of diagonals, and words that occur too often in the
 * set can be left out.
 *
 * The rule (aligner_amd/csrc/aln_seedjoin_rules.h is the rule as code):
 *   parameters  word length k in 1 .. 16, alphabet size A >= 1, A^k <= 2^32 computed in 64 bits (DNA, A = 4: every k; proteins,
 *               A = 20: k <= 7)
 *   word        exactly as in aligner_hip_prefilter.h: a window that touches a code >= A is no word
 *   occurrence  (word, seq, pos), pos the 0-based start of the window in its record.  Every window that is a word is an occurrence;
 *               repeats inside a record count each time
 *   dropped     with max_occ > 0 a word is dropped iff its occurrences in the whole resident set (of a stranded set: all 2n records)
 *               exceed max_occ; a dropped word makes no seed anywhere.  max_occ == 0 drops nothing
 *   seed        for a pair (q, t) of the block every (pq, pt) where the word at (q, pq) equals the word at (t, pt) and is not
 *               dropped; its diagonal is d = pt - pq.  A pair (s, s) of a rectangle is listed like any other (it has its own
 *               pq == pt seeds on d = 0); an upper block has only t > q
 *   band        0 .. 2^31 - 1.  For every diagonal d0 that some seed of the pair has, c(d0) = the seeds of the pair with
 *               d0 <= d <= d0 + band.  seeds(q, t) = max c(d0); diag(q, t) = the least d0 that reaches the maximum
 *   candidate   seeds >= min_seeds, with min_seeds >= 1
 *   order       ascending pair number of the block, as aln_seqset_prefilter and aln_seqset_word_join list them
 * On a mirrored record of a stranded set the positions, and so the diagonal, are in the mirror's own coordinates.
 *
 * aln_seqset_seed_index     builds (or replaces) the resident list of every occurrence of the set -- 12 bytes each, ascending by
 *               (word, sequence) -- and drops any candidate list.  The bitmap index and the word index, if built, stay.
 *               occurrences (optional): how many there are.  ALN_ERR_OOM with nothing changed if the tables cannot be had.  A set of
 *               2^31 residues or more: ALN_ERR_UNSUPPORTED
 * aln_seqset_seed_join      replaces the candidate list with the candidates of `block`.  The result IS the prefilter's candidate
 *               state, `shared` holding seeds: the same resident pair numbers, the same host copy, the same remembered block, the
 *               same limit of 0xFFFFFFF0 candidates (beyond: ALN_ERR_UNSUPPORTED).  aln_seqset_candidates, _candidate_scores,
 *               _candidate_hits and aln_seqset_candidate_best run on it unchanged.  spec->k / alphabet must equal the built seed
 *               index.  The query rows of the block are joined in runs of whole rows of at most chunk_seeds seeds; a single row with
 *               more is ALN_ERR_CAPACITY, decided before anything is changed -- the earlier candidate list, the held hits and all
 *               three indexes stay; max_occ is the remedy.  summary (optional) is written on success
 * aln_seqset_candidate_diags   diag of entries first .. first + n - 1 of a candidate list made by aln_seqset_seed_join.  A list
 *               of aln_seqset_prefilter or aln_seqset_word_join has no diagonals: ALN_ERR_INVALID_ARGUMENT
 *
 * State.  As the prefilter's: the candidate list is separate from the held hits; seed_index and seed_join never touch held hits.
 * aln_seqset_stats: seed_index and seed_join put their kernels' time in ms[2], their wall time in ms[3] and what they moved in bytes[].
 *
 * Refused with ALN_ERR_INVALID_ARGUMENT, nothing written, all state intact: null pointers (occurrences and summary may be null); k or
 * alphabet out of range or A^k beyond 2^32; a spec that does not match the built seed index, or no seed index; min_seeds == 0;
 * band > 2^31 - 1; flags or reserved non-zero; chunk_seeds > 2^26; an invalid block; for aln_seqset_candidate_diags no candidate
 * list, a list of another route, a range beyond the list.
 */
#ifndef ALIGNER_HIP_SEEDJOIN_H
#define ALIGNER_HIP_SEEDJOIN_H
#include "aligner_hip_wordjoin.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct aln_seedjoin_spec {
    uint32_t k, alphabet;          /* offset  0, 4: the seed index the call expects: must equal the built one                 */
    uint32_t min_seeds;            /* offset  8: 1 or more                                                                     */
    uint32_t band;                 /* offset 12: 0 .. 2^31 - 1                                                                 */
    uint32_t max_occ;              /* offset 16: 0: no word is dropped; otherwise words with more occurrences in the set are   */
    uint32_t chunk_seeds;          /* offset 20: 0: 2^24; otherwise 1 .. 2^26 seeds per run of query rows (tuning / tests)     */
    uint32_t flags;                /* offset 24: 0                                                                             */
    uint32_t reserved;             /* offset 28: 0                                                                             */
} aln_seedjoin_spec;               /* 32 bytes */

typedef struct aln_seedjoin_summary {
    uint64_t seeds;                /* offset  0: seeds expanded, over all chunks                  */
    uint64_t pairs_with_seed;      /* offset  8: pairs of the block with at least one seed        */
    uint64_t words_dropped;        /* offset 16: distinct words of the set dropped by max_occ     */
    uint64_t chunks;               /* offset 24: runs of query rows that held a seed              */
} aln_seedjoin_summary;            /* 32 bytes */

int aln_seqset_seed_index(aln_seqset *set, uint32_t k, uint32_t alphabet, uint64_t *occurrences /* optional */);
int aln_seqset_seed_join(aln_seqset *set, const aln_seedjoin_spec *spec, const aln_seqset_block *block, aln_seedjoin_summary *summary /* optional */,
                         uint64_t *count);
int aln_seqset_candidate_diags(aln_seqset *set, uint64_t first, uint64_t n, int32_t *diag);

#ifdef __cplusplus
}
#endif
#endif
