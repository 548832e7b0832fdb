/*
 * aligner_hip_seedchain.h -- seed chains of a resident sequence set: the colinear chain over the seeds of every entry of the candidate
 * list, on the device.  A companion of aligner_hip_seedjoin.h (which it includes): the symbols live in the same libaligner_hip.so,
 * under the same ALN_ABI_VERSION; the other headers' lists are pinned by the project's tests, so this family brings its own header, its
 * own mirror list (_ffi.SEEDCHAIN_EXPORTS) and its own C99 caller (tests/abi_seedchain.c).
 *
 * Why.  A candidate of the seed join says how many seeds its best band of diagonals holds and where that band begins; not where on the
 * two records the match lies, how long it is, or whether the seeds line up in order.  A chain answers that from the integers of the
 * seed index alone, without a fill.
 *
 * The rule (aligner_amd/csrc/aln_seedchain_rules.h is the rule as code):
 *   parameters  k, alphabet must equal the built seed index.  max_occ: the seed join's meaning, over the whole resident set.
 *               max_gap G in 1 .. 2^31 - 1: the largest distance between chained anchors on either record.  max_skew B in
 *               0 .. 2^31 - 1: the largest diagonal drift between chained anchors.  gap_scale g in 0 .. 255: the drift's cost in
 *               sixteenths per base.  max_pair_seeds: 0 means 2^16, else 1 .. 2^20: anchors above which a pair overflows.
 *               chunk_anchors: 0 means 2^24, else 1 .. 2^26: anchors per chunk, for tuning and tests.  flags, reserved: 0
 *   anchors     of a candidate (q, t): exactly the seeds of aligner_hip_seedjoin.h, every (pq, pt) with the same, not dropped, word at
 *               (q, pq) and (t, pt); all of them, not those of one band.  A = their number.  The route that made the list does not
 *               matter: a candidate that shares no word of this index has A = 0
 *   predecessor j is in Pred(i) iff pq_j < pq_i and pt_j < pt_i; pq_i - pq_j <= G and pt_i - pt_j <= G; |dd| <= B with
 *               dd = (pt_i - pt_j) - (pq_i - pq_j), computed in 64 bits.  Pred(i) is a property of the set of anchors, not of any
 *               order they are stored in: there is no "last h predecessors" cut
 *   score       gain(j, i) = min(pq_i - pq_j, pt_i - pt_j, k); cost(j, i) = (|dd| * g) >> 4; v(j, i) = f(j) + gain - cost.
 *               f(i) = v(j*, i) if some j has v(j, i) > k, else k.  j* is the j with the greatest v; equal v by the greatest pq_j,
 *               then the greatest pt_j.  With a predecessor count(i) = count(j*) + 1 and start(i) = start(j*); without one count = 1
 *               and start(i) = (pq_i, pt_i).  f <= k * 2^20 fits int32_t
 *   chain       ends at the anchor e with the greatest f; equal f by the least pq, then the least pt.  score = f(e), anchors =
 *               count(e), q_start / t_start = start(e), q_end = pq_e + k and t_end = pt_e + k, half open, seeds = A
 *   A == 0      every field is 0
 *   overflow    A > max_pair_seeds: the pair is not chained.  flags = ALN_CHAIN_OVERFLOW, seeds = A (0xFFFFFFFF where A is larger
 *               than that) and every other field is 0
 *   filter      keep a candidate iff it overflowed (never lose a pair for being expensive), or score >= min_score and
 *               min(q_end - q_start, t_end - t_start) >= min_span
 * On a mirrored record of a stranded set the positions are in the mirror's coordinates, as diag is.
 *
 * aln_seqset_candidate_chains          chains entries first .. first + n - 1 of the current candidate list, of any route, and writes
 *               n records to the host.  Changes no state.
 * aln_seqset_candidate_chain_filter    chains the whole list and replaces it with the kept entries in their order: index, q, t and
 *               shared travel with their entries, and diag where the list had one; the host copy and the remembered block stay what
 *               the candidate passes expect, so aln_seqset_candidates, _candidate_scores, _candidate_hits and _candidate_best run on
 *               the filtered list unchanged, aln_seqset_candidate_diags keeps answering on a filtered seed-join list and keeps
 *               refusing on the others.  The kept entries' chain records stay resident.  summary (optional) and *count are written
 *               on success.
 * aln_seqset_candidate_chain_records   reads records first .. first + n - 1 of the resident records after a filter; refused where
 *               the current list was not made by a filter.
 *
 * State.  The candidate list is separate from the held hits; none of these calls touches held hits or any of the three indexes.  No
 * result depends on what the handle ran before.  aln_seqset_stats: the kernels' time in ms[2], the wall time in ms[3] and what moved
 * in bytes[]; aln_seqset_candidate_chain_records, like aln_seqset_candidates, leaves the stats of the call before it in place.
 *
 * Refused with ALN_ERR_INVALID_ARGUMENT, nothing written, all state intact: null pointers (summary may be null); no seed index, or a
 * spec whose k / alphabet do not match it; no candidate list; a range beyond the list; max_gap == 0; any field out of its range; flags
 * or reserved non-zero; max_pair_seeds (as given or its default) above chunk_anchors (as given or its default).  A single candidate
 * with more than chunk_anchors anchors that did not overflow would be ALN_ERR_CAPACITY, decided before anything changes; the last
 * refusal keeps max_pair_seeds <= chunk_anchors, so that case cannot arise from a valid spec.  ALN_ERR_OOM leaves the list, the held
 * hits and all three indexes as they were.
 */
#ifndef ALIGNER_HIP_SEEDCHAIN_H
#define ALIGNER_HIP_SEEDCHAIN_H
#include "aligner_hip_seedjoin.h"
#ifdef __cplusplus
extern "C" {
#endif

#define ALN_CHAIN_OVERFLOW 1u      /* aln_chain_record.flags: more anchors than max_pair_seeds, not chained */

typedef struct aln_seedchain_spec {
    uint32_t k, alphabet;          /* offset  0, 4: the seed index the call expects: must equal the built one                   */
    uint32_t max_occ;              /* offset  8: 0: no word is dropped; otherwise words with more occurrences in the set are     */
    uint32_t max_gap;              /* offset 12: G, 1 .. 2^31 - 1                                                                */
    uint32_t max_skew;             /* offset 16: B, 0 .. 2^31 - 1                                                                */
    uint32_t gap_scale;            /* offset 20: g, 0 .. 255: sixteenths per base of drift                                       */
    uint32_t max_pair_seeds;       /* offset 24: 0: 2^16; otherwise 1 .. 2^20                                                    */
    uint32_t chunk_anchors;        /* offset 28: 0: 2^24; otherwise 1 .. 2^26 (tuning / tests); never below max_pair_seeds       */
    uint32_t flags;                /* offset 32: 0                                                                               */
    uint32_t reserved[3];          /* offset 36: 0                                                                               */
} aln_seedchain_spec;              /* 48 bytes */

typedef struct aln_chain_record {
    int32_t score;                 /* offset  0: f(e)                          */
    uint32_t anchors;              /* offset  4: count(e)                      */
    uint32_t q_start;              /* offset  8: start(e).pq                   */
    uint32_t q_end;                /* offset 12: pq_e + k, half open           */
    uint32_t t_start;              /* offset 16: start(e).pt                   */
    uint32_t t_end;                /* offset 20: pt_e + k, half open           */
    uint32_t seeds;                /* offset 24: A                             */
    uint32_t flags;                /* offset 28: 0 or ALN_CHAIN_OVERFLOW       */
} aln_chain_record;                /* 32 bytes */

typedef struct aln_seedchain_summary {
    uint64_t anchors;              /* offset  0: anchors expanded, over all chunks           */
    uint64_t with_anchor;          /* offset  8: candidates with at least one anchor         */
    uint64_t overflowed;           /* offset 16: candidates above max_pair_seeds             */
    uint64_t chunks;               /* offset 24: runs of candidates that held an anchor      */
} aln_seedchain_summary;           /* 32 bytes */

int aln_seqset_candidate_chains(aln_seqset *set, const aln_seedchain_spec *spec, uint64_t first, uint64_t n, aln_chain_record *records,
                                aln_seedchain_summary *summary /* optional */);
int aln_seqset_candidate_chain_filter(aln_seqset *set, const aln_seedchain_spec *spec, int32_t min_score, uint32_t min_span,
                                      aln_seedchain_summary *summary /* optional */, uint64_t *count);
int aln_seqset_candidate_chain_records(aln_seqset *set, uint64_t first, uint64_t n, aln_chain_record *records);

#ifdef __cplusplus
}
#endif
#endif
