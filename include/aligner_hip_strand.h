/*
 * aligner_hip_strand.h -- the strand calls of the C ABI: a resident sequence set that holds every record on both strands, the second
 * one made on the device, and the CIGARs of its held hits with the coordinates and the word order a PAF line or a SAM record wants for
 * a hit on the minus strand.  A companion of aligner_hip_cigar.h (which it includes): the symbols live in the same libaligner_hip.so,
 * under the same ALN_ABI_VERSION.
 *
 * Why another header: the project's tests pin the lists of functions and records of the headers before it.  This family brings its own
 * header, its own mirror list (_ffi.STRAND_EXPORTS) and its own C99 caller (tests/abi_strand.c).
 *
 * aligner_amd/csrc/aln_strand_rules.h is the rule as code.  In words:
 *   the set     aln_seqset_create_stranded takes n records and holds 2n: records 0 .. n - 1 are the caller's, record n + i is the mirror
 *               of record i, mirror[j] = map[rec[len - 1 - j]], of the same length.  Only the n forward records go up (and the 256
 *               bytes of map); one kernel writes the mirrors behind them in the set's one residue buffer, off[n + i] = total + off[i]
 *               with total the residues of the n records.  The buffer has 2 * total + 256 bytes from the start and never moves.
 *               map is any byte table: it is not validated and need not be an involution.  code ^ 1 for the codes 0 .. 3 of A, T, C, G
 *               is the complement; the identity gives plain reversal for any alphabet
 *   its calls   every aln_seqset_* call takes the 2n records as ordinary records and knows nothing of strands: a block q in [0, n) x
 *               t in [n, 2n) is the minus-strand rectangle, q in [0, n) x t in [0, 2n) both strands in one pass, one row per query
 *   a hit       of records (q_seq, t_seq) of the 2n: qm = q_seq >= n, tm = t_seq >= n; q_rec = q_seq mod n, t_rec = t_seq mod n; strand
 *               '-' iff qm != tm
 *   the record  aln_cigar_record of the plain plan for the same hit and flags, but with the coordinates on the original records:
 *               qm: (q_start, q_end) = (N - q_end, N - q_start); tm: (t_start, t_end) = (M - t_end, M - t_start), N and M the two
 *               lengths.  n_ops, matches, block and status are the plain plan's; a hit whose status is not ALN_OK keeps its all-zero
 *               record
 *   the words   those of the plain plan, in reverse order iff tm: PAF and SAM give a CIGAR along the forward target.  The ops do not
 *               change -- query and target keep their roles -- and with ALN_CIGAR_CLIPS the leading and the trailing clip change
 *               places with the rest.  Word r of the plain plan is word n_ops - 1 - r
 *   the rest    the offsets, the summary and every refusal are the plain plan's
 *
 * aln_seqset_held_strand_cigar_plan / _fill are aln_seqset_held_cigar_plan / _fill with that rule; up goes one more byte per listed hit,
 * down comes what the plain plan brings (the strand records are the host's).  The two families share the set's tables and its one "last plan": a plan of either family replaces the plan before
 * it, whichever family that was, and a fill answers only a plan of its own family -- after a plan of the other it is refused like a
 * fill without a plan.  A refusal leaves the plan before it intact.
 * aln_seqset_strand_records gives n of a stranded set, 0 for a plain set or NULL.
 * aln_seqset_strand_residues brings down records first .. first + count - 1 of the resident 2n (of any set: n of a plain one), record
 * first + k to out + out_off[k]: what the mirror kernel wrote, for tests and for callers that want the mirror's bytes.
 *
 * Refused, nothing created or written: aln_seqset_create_stranded -- a null map or any null-pointer case of aln_seqset_create
 * (ALN_ERR_INVALID_ARGUMENT), 2 * n_seqs >= 2^32 (ALN_ERR_INVALID_ARGUMENT), a record longer than 0x7FFFFFF0 (ALN_ERR_UNSUPPORTED).
 * The plan -- what aln_seqset_held_cigar_plan refuses, a null `strands` (n != 0), a set that is not stranded
 * (ALN_ERR_INVALID_ARGUMENT).  The fill -- what aln_seqset_held_cigar_fill refuses, a last plan of the other family.
 * aln_seqset_strand_residues -- a null set, a null out_off (count != 0), a null out where a listed record has residues, a range beyond
 * the set's records (ALN_ERR_INVALID_ARGUMENT).
 *
 * Not built: strand folding inside aln_seqset_best (a record may appear on both strands among a query's K); clusters, profiles and
 * family alignments over stranded hits (they would see 2n unrelated records); a block shape for "i < j across strands".
 */
#ifndef ALIGNER_HIP_STRAND_H
#define ALIGNER_HIP_STRAND_H
#include "aligner_hip_cigar.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct aln_strand_record {
    uint32_t q_rec;        /* offset  0: q_seq mod n                                          */
    uint32_t t_rec;        /* offset  4: t_seq mod n                                          */
    uint8_t strand;        /* offset  8: '+' or '-'                                           */
    uint8_t q_mirror;      /* offset  9: 1 iff q_seq >= n                                     */
    uint8_t t_mirror;      /* offset 10: 1 iff t_seq >= n: the words are in reverse order     */
    uint8_t reserved;      /* offset 11: 0                                                    */
    uint32_t reserved2;    /* offset 12: 0                                                    */
} aln_strand_record;       /* 16 bytes */

aln_seqset *aln_seqset_create_stranded(aln_ctx *ctx, const uint8_t *seqs, const uint64_t *off, const uint64_t *len, size_t n_seqs,
                                       const uint8_t map[256], int *status);
uint64_t aln_seqset_strand_records(const aln_seqset *set);
int aln_seqset_strand_residues(aln_seqset *set, uint64_t first, uint64_t count, const uint64_t *out_off /* count */, uint8_t *out);

int aln_seqset_held_strand_cigar_plan(aln_seqset *set, uint32_t flags, const uint32_t *which /* n */, uint64_t n, aln_cigar_record *records /* n */,
                                      aln_strand_record *strands /* n */, aln_cigar_summary *summary);
int aln_seqset_held_strand_cigar_fill(aln_seqset *set, uint32_t *ops /* capacity_ops */, uint64_t capacity_ops, uint64_t *offsets /* n + 1, optional */,
                                      uint64_t capacity_offsets);

#ifdef __cplusplus
}
#endif
#endif
