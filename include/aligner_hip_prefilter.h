/*
 * aligner_hip_prefilter.h -- the k-mer prefilter of a resident sequence set: count the short words two sequences share first, run
 * the dynamic programme only on the pairs that share enough of them.  A companion of aligner_hip.h (which it includes), as
 * aligner_hip_cluster.h is: the symbols live in the same libaligner_hip.so, under the same ALN_ABI_VERSION; the main header's list
 * is pinned by the project's tests, so this family brings its own header, its own mirror list (_ffi.PREFILTER_EXPORTS) and its own
 * C99 caller (tests/abi_prefilter.c).
 *
 * The prefilter is opt-in and exact in what it promises: the alignments of the surviving pairs are bit for bit those of the
 * unfiltered pass, and which pairs survive follows an integer rule (aligner_amd/csrc/aln_prefilter_rules.h is the rule as code):
 *   parameters  word length k in 1 .. 8, alphabet size A >= 1, A^k <= 2^18 (proteins, the twenty standard residues first: A = 20,
 *               k <= 4; DNA, A = 4: every k)
 *   word        a window s[i .. i + k - 1] in which ALL codes are < A; its number is sum c_j A^(k-1-j).  A window that touches a code
 *               >= A is no word.  K(s) is the SET of word numbers of s, n(s) = |K(s)|; a sequence shorter than k has n = 0
 *   shared      shared(q, t) = |K(q) & K(t)|
 *   candidate   shared >= min_shared  and  shared * 1024 >= min_per_1024 * min(n(q), n(t)), in uint64_t arithmetic;
 *               min_per_1024 in 0 .. 1024.  With both thresholds 0 every pair of the block is a candidate
 *   bitmap      what the device keeps per sequence: (A^k + 31) / 32 32-bit elements, word w is bit w & 31 of element w >> 5
 *
 * aln_seqset_kmer_index     builds (or replaces) the resident bitmaps and word counts of every sequence of the set and drops any
 *               candidate list.  n_words (optional): n(s) of every sequence.  ALN_ERR_OOM with nothing changed if the table cannot
 *               be had
 * aln_seqset_prefilter      replaces the candidate list with the candidates of `block`, ascending in pair number.  The list stays
 *               resident (8 bytes of pair number per candidate); a copy with `shared` comes down (12 bytes per candidate), from which
 *               the host plans the later passes.  *count is exact.  spec->k / alphabet must equal the built index.  More than
 *               0xFFFFFFF0 candidates: ALN_ERR_UNSUPPORTED.  The block is remembered
 * aln_seqset_candidates     candidates first .. first + n - 1 from the host copy: pair number in the block, sequence numbers, shared
 * aln_seqset_candidate_scores   a pass like aln_seqset_score over the candidate list instead of the block: f[c] and status[c]
 *               (optional) belong to candidate c.  Per-pair failures and the return value without status are aln_seqset_score's
 * aln_seqset_candidate_hits     the same pass with the threshold selection of aln_seqset_hits: the candidates with status ALN_OK and
 *               f >= f_min are held exactly as aln_seqset_hits would hold those pairs: aln_seqset_held_list reports their pair
 *               numbers in the prefilter's block, and held_strings, held_report, held_filter, held_significance and held_cluster
 *               work unchanged on top
 *
 * State.  The candidate list is separate from the held hits: it survives score, hits, best and the held calls and ends at the next
 * kmer_index, prefilter or destroy.  kmer_index, prefilter and candidates leave held hits untouched; the two candidate passes start
 * like any pass (earlier held hits are gone, the stats are reset).  aln_seqset_stats: the two passes fill ms[] and bytes[] as score and
 * hits do; kmer_index and prefilter put their kernels' time in ms[2], their wall time in ms[3] and what they moved in bytes[].
 *
 * Refused with ALN_ERR_INVALID_ARGUMENT, nothing written, all state intact: null pointers; k or alphabet out of range or A^k beyond
 * the cap; a spec that does not match the built index, or no index; min_per_1024 > 1024; flags or reserved non-zero; chunk_pairs >
 * 2^22; an invalid block; no candidate list; first + n > count.  ALN_PWM_LOCAL params: ALN_ERR_UNSUPPORTED.
 */
#ifndef ALIGNER_HIP_PREFILTER_H
#define ALIGNER_HIP_PREFILTER_H
#include "aligner_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct aln_prefilter_spec {
    uint32_t k, alphabet;          /* offset  0, 4: the index the call expects: must equal the built one                        */
    uint32_t min_shared;           /* offset  8                                                                                  */
    uint32_t min_per_1024;         /* offset 12: 0 .. 1024                                                                       */
    uint32_t chunk_pairs;          /* offset 16: 0: 2^22; otherwise 1 .. 2^22 pairs per sharing chunk (tuning / tests)           */
    uint32_t flags;                /* offset 20: 0                                                                               */
    uint64_t reserved;             /* offset 24: 0                                                                               */
} aln_prefilter_spec;              /* 32 bytes */

int aln_seqset_kmer_index(aln_seqset *set, uint32_t k, uint32_t alphabet, uint32_t *n_words /* optional, n_seqs */);
int aln_seqset_prefilter(aln_seqset *set, const aln_prefilter_spec *spec, const aln_seqset_block *block, uint64_t *count);
int aln_seqset_candidates(aln_seqset *set, uint64_t first, uint64_t n, uint64_t *pair_index, uint32_t *q_seq, uint32_t *t_seq,
                          uint32_t *shared);
int aln_seqset_candidate_scores(aln_seqset *set, const aln_params *params, double *f, int32_t *status /* optional */);
int aln_seqset_candidate_hits(aln_seqset *set, const aln_params *params, double f_min, uint64_t *count);

#ifdef __cplusplus
}
#endif
#endif
