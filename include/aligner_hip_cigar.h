/*
 * aligner_hip_cigar.h -- the CIGAR calls of the C ABI: the pairwise alignments of a resident sequence set's held hits, run-length
 * encoded on the device from their aligned strings, with the coordinates a PAF line or a SAM record needs beside them.  A companion of
 * aligner_hip.h (which it includes): the symbols live in the same libaligner_hip.so, under the same ALN_ABI_VERSION.
 *
 * Why another header: the project's tests pin the lists of functions and records of the headers before it.  This family brings its own
 * header, its own mirror list (_ffi.CIGAR_EXPORTS) and its own C99 caller (tests/abi_cigar.c).
 *
 * aligner_amd/csrc/aln_cigar_rules.h is the rule as code.  In words, with which[n] the listed positions of the held list exactly as
 * aln_seqset_held_report takes them (any order, repeats allowed) and blank the blank code of the held pass:
 *   columns     the first aln_report_columns(aln_len, ALN_REPORT_SKIP_SEED) columns of the hit's two strings, x = query[j] and
 *               y = target[j] as held_strings returns them: the traceback's duplicated seed column is never part of a CIGAR.  n columns
 *   op          SAM's numbering, so that the words are BAM's.  Both non-blank: M (0), or with ALN_CIGAR_EXTENDED = (7) if x == y, else
 *               X (8).  x non-blank, y blank: I (1), consumes the query only.  x blank, y non-blank: D (2), consumes the target only.
 *               Both blank: P (6), SAM's padding, consumes neither (not in strings that are the set's own; no column is special)
 *   runs        a run is a maximal stretch of counted columns with the same op: one word length << 4 | op, in column order.  Column
 *               n - 1 always ends a run; the seed column at index n is never looked at
 *   clips       only with ALN_CIGAR_CLIPS, zero-length clips omitted: a leading S (4) of start_x first, a trailing S of N - q_end last
 *               (N: the query's length).  q_end > N: no trailing clip, one more in summary->overflow (not for the set's own strings).
 *               A clip's length is held at 2^28 - 1 (a start_x beyond that is not a coordinate of a supported set)
 *   record      n_ops runs plus clips; q_start = start_x, q_end = start_x + the query non-blanks among the counted columns; t_start =
 *               start_y, t_end alike over the target (the ends in 64 bits, saturated to 32); matches: columns with x == y != blank
 *               (PAF column 10); block: counted columns that are not P (PAF column 11); status: the held entry's.  A held entry whose
 *               status is not ALN_OK gets an all-zero record with that status and no ops
 *   layout      listed hit k's words start at word off[k] = the sum of n_ops of the listed hits before it, in 64 bits; off[n] =
 *               summary->total_ops
 *   summary     held: the held hits; listed: n; total_ops; failed: listed entries whose status is not ALN_OK; padded: P columns of
 *               the listed hits; overflow: as above (the three saturate at 2^32 - 1)
 *
 * aln_seqset_held_cigar_plan counts and classes every listed hit, turns n_ops into the 64-bit offsets on the device and brings down one
 * record per listed hit (32 bytes) and the counters; up go the listed positions (4 bytes each).  The offsets, the listed positions and
 * the flags stay with the set, on the device, until the next plan.
 * aln_seqset_held_cigar_fill writes the words of the last plan and brings them down (4 * total_ops bytes), with a non-null `offsets` also
 * the n + 1 word offsets (8 bytes each); nothing goes up and nothing is decided again.  It may be called more than once; every call
 * gives the same bytes.
 * Both run on the set's stream into buffers of their own: the held summaries, strings and list and the report buffer are not written,
 * and every other held call answers afterwards as before.  stats: ms[2] the call's kernels, ms[3] its wall time; ms[0] and ms[1] stay
 * the held pass's.
 *
 * Refused with ALN_ERR_INVALID_ARGUMENT, nothing written, all state intact (an earlier plan too) -- the plan: a flag bit other than the
 * two, a null set, `which` (n != 0), records (n != 0) or summary, no held hits, n beyond 0x7FFFFFF0, a listed position beyond the held
 * hits; the fill: no plan, a held pass on the set since the plan, capacity_ops below total_ops, a non-null `offsets` with
 * capacity_offsets below n + 1, a null `ops` where total_ops is not 0.
 * ALN_ERR_UNSUPPORTED (the plan): a set in which some N + M + 2 reaches 2^28 -- a run must fit 28 bits.
 */
#ifndef ALIGNER_HIP_CIGAR_H
#define ALIGNER_HIP_CIGAR_H
#include "aligner_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define ALN_CIGAR_EXTENDED 1u  /* = and X in place of M                                           */
#define ALN_CIGAR_CLIPS 2u     /* soft clips for the query's residues outside the alignment       */

/* SAM's op numbers (the low four bits of a word) */
#define ALN_CIGAR_M 0u
#define ALN_CIGAR_I 1u
#define ALN_CIGAR_D 2u
#define ALN_CIGAR_S 4u
#define ALN_CIGAR_P 6u
#define ALN_CIGAR_EQ 7u
#define ALN_CIGAR_X 8u

typedef struct aln_cigar_record {
    uint32_t n_ops;        /* offset  0: runs plus clips                                      */
    uint32_t q_start;      /* offset  4: start_x                                              */
    uint32_t q_end;        /* offset  8                                                       */
    uint32_t t_start;      /* offset 12: start_y                                              */
    uint32_t t_end;        /* offset 16                                                       */
    uint32_t matches;      /* offset 20: PAF column 10                                        */
    uint32_t block;        /* offset 24: PAF column 11                                        */
    int32_t status;        /* offset 28: the held entry's                                     */
} aln_cigar_record;        /* 32 bytes */

typedef struct aln_cigar_summary {
    uint64_t held;             /* offset  0: the held hits                                    */
    uint64_t listed;           /* offset  8: n                                                */
    uint64_t total_ops;        /* offset 16: the words of all listed hits                     */
    uint32_t failed;           /* offset 24: listed entries whose status is not ALN_OK        */
    uint32_t padded;           /* offset 28: P columns                                        */
    uint32_t overflow;         /* offset 32: q_end beyond the query's length                  */
    uint32_t reserved[3];      /* offset 36: 0                                                */
} aln_cigar_summary;           /* 48 bytes */

int aln_seqset_held_cigar_plan(aln_seqset *set, uint32_t flags, const uint32_t *which /* n */, uint64_t n, aln_cigar_record *records /* n */,
                               aln_cigar_summary *summary);
int aln_seqset_held_cigar_fill(aln_seqset *set, uint32_t *ops /* capacity_ops */, uint64_t capacity_ops, uint64_t *offsets /* n + 1, optional */,
                               uint64_t capacity_offsets);

#ifdef __cplusplus
}
#endif
#endif
