/*
 * aligner_hip_profile.h -- the profile family of the C ABI: per-position residue counts of the families of a resident sequence set,
 * counted on the device over the aligned strings of its held hits.  A companion of aligner_hip_cluster.h (which it includes): the
 * symbols live in the same libaligner_hip.so, under the same ALN_ABI_VERSION.
 *
 * Why another header: the project's tests pin the lists of functions and records of the headers before it (their number, the mirror
 * lists of the bindings, the C99 callers).  This family was added without moving those yardsticks, so it brings its own header, its
 * own mirror list (_ffi.PROFILE_EXPORTS) and its own C99 caller (tests/abi_profile.c).
 *
 * aligner_amd/csrc/aln_profile_rules.h is the rule as code.  In words, for a set of S sequences with held hits (of aln_seqset_hits,
 * aln_seqset_best or the candidate passes):
 *   label       S words, one per sequence: aln_seqset_held_cluster's labels, or any labelling of the caller's.  ALN_CLUSTER_NONE is
 *               allowed; a label is never used as an index
 *   centers     n_centers strictly ascending sequence numbers below S: the sequences that get a profile
 *   who counts  a held hit (q, t) contributes iff its status is ALN_OK, with a filter aln_report_keep keeps its report (params, flags
 *               and filter as aln_seqset_held_cluster takes them), q != t, label[q] == label[t] != ALN_CLUSTER_NONE, and exactly one
 *               of q, t equals that label: the centre c; the other is the member.  A pair listed in both orientations contributes
 *               twice.  Of the hits that are ALN_OK (and kept) but do not contribute: q == t is a self pair; the same label on both
 *               ends and neither end is it: between members; a centre that `centers` does not list: unlisted.  Every other hit
 *               (different labels, ALN_CLUSTER_NONE) is counted nowhere
 *   columns     the first aln_report_columns(aln_len, flags) columns of the hit's two aligned strings: all, or with
 *               ALN_PROFILE_SKIP_SEED (== ALN_REPORT_SKIP_SEED) all but the last, the traceback's duplicated seed pair
 *   positions   the centre's string is the aligned query if q == c, else the aligned target; its first residue sits at centre position
 *               start_x (start_y) of the hit's summary, 0-based.  The i-th non-blank of the centre's string (i from 0) sits at
 *               start + i.  The seed column, when it is counted, repeats the end cell's residue: it sits at the position of the
 *               non-blank before it, start + i - 1 (start if there is none)
 *   rows        a profile has R = n_codes + 2 rows and len[c] columns, row-major [row][position], uint32_t.  A counted column with
 *               centre code cc and member code mc: cc == blank: nothing (an insert relative to the centre); mc < n_codes: row mc;
 *               mc == blank: row n_codes, a deletion; any other mc: row n_codes + 1.  One is added per column, so the sum of a
 *               profile's column is the number of contributing hits that cover that position (plus the seed columns that land on it)
 *   blank       params->blank_code with a filter, else the blank code of the held pass
 *   overflow    a position >= len[c] is never written; it is counted in summary->overflow (0 for strings that are the set's own)
 *   layout      profile i starts at element sum over j < i of R * len[centers[j]]; aln_seqset_profile_elements gives the total
 *   records     one per centre, in the order of `centers`: the centre, its contributing hits, the counts in rows < n_codes, the
 *               counts in row n_codes
 *
 * aln_seqset_profile_elements: *total = the elements all profiles of `centers` take.  Host arithmetic only; no held pass is needed.
 * aln_seqset_held_profiles: up go the hits' endpoints (8 bytes per held hit), the labels (4 per sequence), the centres and their
 * offsets (12 per centre), with a filter the bit table; down come 4 bytes per element, 16 per centre and the counters.  The output is
 * zeroed on the device and counted there with integer adds, so every number is independent of the order anything ran in.  The call
 * runs on the set's stream into buffers of its own: the held summaries, strings and list are not written, and held_list,
 * held_strings, held_report, held_filter, held_significance and held_cluster answer afterwards as before (with a filter the set's
 * report buffer is rewritten, as held_filter and held_cluster do).  stats: ms[2] this call's kernels, ms[3] its wall time, bytes[]
 * as above; ms[0] and ms[1] stay the held pass's.  hits, matched and deleted of a record are 32-bit sums.
 *
 * Refused with ALN_ERR_INVALID_ARGUMENT, nothing written, all state intact: a null set, label (S > 0), summary, total, centers or
 * records (n_centers > 0) or out (elements > 0); centres not strictly ascending or not below S; n_codes outside 1 .. 64; a flag bit
 * other than ALN_PROFILE_SKIP_SEED; capacity_elements below the total; a filter without params or params without a filter;
 * filter->reserved != 0; no held pass; and what aln_seqset_held_filter refuses of params.  ALN_PWM_LOCAL params, rows * cols > 8192:
 * ALN_ERR_UNSUPPORTED.  Host memory that cannot be had: ALN_ERR_OOM.
 */
#ifndef ALIGNER_HIP_PROFILE_H
#define ALIGNER_HIP_PROFILE_H
#include "aligner_hip_cluster.h"
#ifdef __cplusplus
extern "C" {
#endif

#define ALN_PROFILE_SKIP_SEED 1u          /* == ALN_REPORT_SKIP_SEED */
#define ALN_PROFILE_MAX_CODES 64u

typedef struct aln_profile_record {
    uint32_t center;       /* the sequence number                                             */
    uint32_t hits;         /* contributing hits                                               */
    uint32_t matched;      /* counts in rows < n_codes                                        */
    uint32_t deleted;      /* counts in row n_codes                                           */
} aln_profile_record;      /* 16 bytes */

typedef struct aln_profile_summary {
    uint64_t held;             /* offset  0: the held hits                                    */
    uint64_t contributing;     /* offset  8                                                   */
    uint32_t self_pairs;       /* offset 16                                                   */
    uint32_t between_members;  /* offset 20                                                   */
    uint32_t unlisted;         /* offset 24                                                   */
    uint32_t overflow;         /* offset 28: columns at a position >= len[c] (saturating)     */
    uint64_t elements;         /* offset 32: the total of aln_seqset_profile_elements         */
    uint64_t reserved;         /* offset 40: 0                                                */
} aln_profile_summary;         /* 48 bytes */

int aln_seqset_profile_elements(const aln_seqset *set, const uint32_t *centers, uint64_t n_centers, uint32_t n_codes, uint64_t *total);
int aln_seqset_held_profiles(aln_seqset *set, const aln_params *params /* optional */, uint32_t flags, const aln_hit_filter *filter /* optional */,
                             const uint32_t *label /* n_seqs */, const uint32_t *centers, uint64_t n_centers, uint32_t n_codes,
                             uint32_t *out /* capacity_elements */, uint64_t capacity_elements, aln_profile_record *records /* n_centers */,
                             aln_profile_summary *summary);

#ifdef __cplusplus
}
#endif
#endif
