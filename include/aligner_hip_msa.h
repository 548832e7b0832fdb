/*
 * aligner_hip_msa.h -- the family-alignment calls of the C ABI: a centre-star multiple alignment of every family of a resident sequence
 * set, laid out and written on the device from the aligned strings of its held hits.  A companion of aligner_hip_profile.h (which it
 * includes): the symbols live in the same libaligner_hip.so, under the same ALN_ABI_VERSION.
 *
 * Why another header: the project's tests pin the lists of functions and records of the headers before it.  This family brings its own
 * header, its own mirror list (_ffi.MSA_EXPORTS) and its own C99 caller (tests/abi_msa.c).
 *
 * aligner_amd/csrc/aln_msa_rules.h is the rule as code.  In words, with label, centers, params and filter as aln_seqset_held_profiles
 * takes them (there is no n_codes, and flags must be 0):
 *   who         a held hit contributes iff it contributes to a profile: status ALN_OK, with a filter kept, q != t, both ends carry the
 *               same label != ALN_CLUSTER_NONE, exactly one end is that label (the centre c) and `centers` lists c.  self_pairs,
 *               between_members and unlisted count what they count there.  A pair held in both orientations gives two rows
 *   columns     the first aln_report_columns(aln_len, ALN_REPORT_SKIP_SEED) columns of the hit's two strings: the traceback's duplicated
 *               seed column is never part of a family alignment.  With a filter the reports are classed over the same columns
 *   positions   the i-th non-blank of the centre's string sits at centre position p = start + i (start_x if q == c, else start_y),
 *               computed in 64 bits
 *   inserts     a maximal run of counted columns whose centre code is blank, with b centre non-blanks in front of it, is an insert
 *               before centre position p = start + b, p in 0 .. len[c] (p == len[c]: after the last residue).  ins[p] is the longest
 *               such run of any contributing hit of c, 0 without one
 *   columns of  centre position p stands in column col(p) = p + ins[0] + ... + ins[p]; the insert block before p is columns
 *   the family  col(p) - ins[p] .. col(p) - 1; the block after the last residue W - ins[len] .. W - 1; W = len[c] + the sum of all ins.
 *               The k-th column of a run (k from 0) goes to the k-th column of its block: inserts are left-justified
 *   rows        row 0 is the centre: its residue p at col(p), blank elsewhere.  Rows 1 .. rows are the contributing hits of c in
 *               ascending held position: the member's code at every counted column of the hit, blank everywhere else (the flanks of
 *               a local alignment too)
 *   layout      family i is a row-major uint8_t matrix of (rows_i + 1) x width_i at byte sum over j < i of (rows_j + 1) * width_j of
 *               `out`; its row list starts at entry sum over j < i of (rows_j + 1) of `row_hit`: the held position of every row,
 *               ALN_CLUSTER_NONE for row 0
 *   overflow    a residue column at p >= len[c] and a column of an insert at p > len[c] are neither measured nor written; they are
 *               counted in summary->overflow (0 for strings that are the set's own)
 *   blank       params->blank_code with a filter, else the blank code of the held pass
 *
 * aln_seqset_held_msa_plan decides who contributes, measures the inserts, lays the columns out and brings down one record per centre
 * (16 bytes) and the counters; the plan stays with the set, on the device, until the next plan.  Up go the hits' endpoints (8 bytes per
 * held hit), the labels (4 per sequence), the centres and the offsets of their tables (12 per centre), with a filter the bit table.
 * summary->bytes and summary->total_rows are the sizes the fill needs.
 * aln_seqset_held_msa_fill writes the matrices and row lists of the last plan and brings them down: bytes + 4 * total_rows bytes, nothing
 * up.  It decides nothing again.  It may be called more than once; every call gives the same bytes.
 * Both run on the set's stream into buffers of their own: the held summaries, strings and list are not written, and held_list,
 * held_strings, held_report, held_filter, held_significance, held_cluster and held_profiles answer afterwards as before (with a filter
 * the set's report buffer is rewritten, as held_filter does).  stats: ms[2] the call's kernels, ms[3] its wall time, bytes[] as above;
 * ms[0] and ms[1] stay the held pass's.
 *
 * Refused with ALN_ERR_INVALID_ARGUMENT, nothing written, all state intact (an earlier plan too) -- the plan: what
 * aln_seqset_held_profiles refuses of the set, label, centers, records, summary, params and filter, and flags != 0; the fill: no plan, a
 * held pass on the set since the plan, capacity_bytes or capacity_rows below the plan's totals, a null buffer where the total is not 0.
 * ALN_ERR_UNSUPPORTED: ALN_PWM_LOCAL params, rows * cols > 8192, a width or a row count that does not fit 32 bits.
 */
#ifndef ALIGNER_HIP_MSA_H
#define ALIGNER_HIP_MSA_H
#include "aligner_hip_profile.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct aln_msa_record {
    uint32_t center;       /* the sequence number                                             */
    uint32_t rows;         /* contributing hits: the matrix has rows + 1 rows                 */
    uint32_t width;        /* the columns of the matrix                                       */
    uint32_t inserted;     /* width - len[center]                                             */
} aln_msa_record;          /* 16 bytes */

typedef struct aln_msa_summary {
    uint64_t held;             /* offset  0: the held hits                                    */
    uint64_t contributing;     /* offset  8                                                   */
    uint32_t self_pairs;       /* offset 16                                                   */
    uint32_t between_members;  /* offset 20                                                   */
    uint32_t unlisted;         /* offset 24                                                   */
    uint32_t overflow;         /* offset 28: columns beyond the centre (saturating)           */
    uint64_t bytes;            /* offset 32: all matrices                                     */
    uint64_t total_rows;       /* offset 40: the sum of rows + 1                              */
} aln_msa_summary;             /* 48 bytes */

int aln_seqset_held_msa_plan(aln_seqset *set, const aln_params *params /* optional */, uint32_t flags /* 0 */, const aln_hit_filter *filter /* optional */,
                             const uint32_t *label /* n_seqs */, const uint32_t *centers, uint64_t n_centers, aln_msa_record *records /* n_centers */,
                             aln_msa_summary *summary);
int aln_seqset_held_msa_fill(aln_seqset *set, uint8_t *out /* capacity_bytes */, uint64_t capacity_bytes, uint32_t *row_hit /* capacity_rows */,
                             uint64_t capacity_rows);

#ifdef __cplusplus
}
#endif
#endif
