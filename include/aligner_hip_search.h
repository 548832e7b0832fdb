/*
 * aligner_hip_search.h -- the k best partners per record over a prefiltered candidate list: the database-search question of
 * aln_seqset_best asked of the pairs that aln_seqset_prefilter kept, so that only those are aligned.  A companion of
 * aligner_hip_prefilter.h (which it includes), as that header is one of aligner_hip.h: the symbol lives in the same
 * libaligner_hip.so, under the same ALN_ABI_VERSION; the other headers' lists are pinned by the project's tests, so this call brings
 * its own header, its own mirror list (_ffi.SEARCH_EXPORTS) and its own C99 caller (tests/abi_search.c).
 *
 * The rule is aln_seqset_best's, restricted to the list (aligner_amd/csrc/aln_best_rules.h and aln_search_rules.h are the rule as
 * code):
 *   selectable  an entry of the candidate list whose alignment has status ALN_OK, f == f and f >= f_min (plain IEEE compares: a NaN
 *               f_min selects nothing); with ALN_BEST_SKIP_SELF also q != t as sequence numbers.  A self pair on the list is aligned
 *               and then skipped
 *   order       (f, t) comes before (f', t') iff f > f', or f == f' and t < t'.  -0.0 == +0.0
 *   kept        of every query row of the prefilter's rectangle the first min(k, t_count) of its selectable entries under the order.
 *               The order is total, so the result depends on neither chunking nor launch geometry
 *   geometry    the list L holds ascending pair numbers of a rectangle with T = t_count targets per row.  Entry i belongs to row
 *               L[i] / T, its target is t_first + L[i] % T, its query q_first + L[i] / T.  Row r's entries are the list positions
 *               row_first[r] .. row_first[r + 1] - 1, where row_first[r] counts the entries below r * T; a row may have none.  The
 *               device cuts a chunk of list positions into pieces of 2048 POSITIONS, not by row: a piece usually holds many short
 *               rows, a long row spans several pieces, and because the list ascends a piece sorted by (row, order) keeps every row's
 *               run where it was
 *
 * aln_seqset_candidate_best   aligns the candidates (the pass of aln_seqset_candidate_scores), selects per row on the device and holds
 *               the kept pairs exactly as aln_seqset_best would hold those pairs: *count is their number, aln_seqset_held_list
 *               reports them in ascending pair number of the prefilter's block (16 bytes per kept pair come down), and held_strings,
 *               held_report, held_filter, held_significance and held_cluster work unchanged on top.  k in 1 .. ALN_SEQSET_BEST_MAX
 *
 * State.  The call starts like any pass (earlier held hits are gone, the stats are reset); the candidate list survives it.
 * aln_seqset_stats: ms[0] the fill, ms[1] the re-fill of the kept pairs, ms[2] the selection kernels, ms[3] the wall time; bytes[] as
 * aln_seqset_best counts them.
 *
 * Refused with nothing written and all state intact: a null set, params or count, k outside 1 .. ALN_SEQSET_BEST_MAX, flag bits
 * other than ALN_BEST_SKIP_SELF, no candidate list: ALN_ERR_INVALID_ARGUMENT.  A candidate list made on an upper block (a pair of
 * it belongs to both of its sequences), ALN_PWM_LOCAL params: ALN_ERR_UNSUPPORTED.  An empty candidate list holds nothing: count 0.
 */
#ifndef ALIGNER_HIP_SEARCH_H
#define ALIGNER_HIP_SEARCH_H
#include "aligner_hip_prefilter.h"
#ifdef __cplusplus
extern "C" {
#endif

int aln_seqset_candidate_best(aln_seqset *set, const aln_params *params, uint32_t k, double f_min, uint32_t flags, uint64_t *count);

#ifdef __cplusplus
}
#endif
#endif
