// aln_seedchain_rules.h -- the colinear chain over the seeds of a candidate of a resident sequence set (aln_seqset_candidate_chains /
// _chain_filter, include/aligner_hip_seedchain.h) as plain integer code, no HIP: the kernels (aln_seedchain.hip), the host
// (aln_host.hip) and a CPU test driver decide with the same lines which specs are taken, which anchor may precede which, what a link
// is worth, which predecessor and which end win a tie, what a record holds and which records a filter keeps.
//
//   parameters  k, alphabet: the built seed index's.  max_occ: the seed join's.  max_gap G in 1 .. 2^31 - 1, max_skew B in
//               0 .. 2^31 - 1, gap_scale g in 0 .. 255 (sixteenths per base), max_pair_seeds 0 (2^16) or 1 .. 2^20, chunk_anchors 0
//               (2^24) or 1 .. 2^26 and never below max_pair_seeds, flags and reserved 0
//   anchors     of a candidate (q, t): the seeds of aln_seedjoin_rules.h, all of them: every (pq, pt) with the same, not dropped, word
//               at (q, pq) and (t, pt).  A = their number.  Positions are below 2^31
//   predecessor j in Pred(i) iff pq_j < pq_i and pt_j < pt_i; pq_i - pq_j <= G and pt_i - pt_j <= G; |dd| <= B with
//               dd = (pt_i - pt_j) - (pq_i - pq_j) in 64 bits.  A property of the set of anchors, not of their stored order
//   score       gain(j, i) = min(pq_i - pq_j, pt_i - pt_j, k); cost(j, i) = (|dd| * g) >> 4; v(j, i) = f(j) + gain - cost in 64 bits.
//               f(i) = v(j*, i) if some j has v(j, i) > k, else k.  j*: the greatest v; equal v by the greatest pq_j, then the
//               greatest pt_j.  With a predecessor count(i) = count(j*) + 1 and start(i) = start(j*); without: 1 and (pq_i, pt_i)
//   range       a chain has at most max_pair_seeds <= 2^20 anchors and every link adds at most k <= 16, so f <= k * 2^20 <= 2^24:
//               int32_t holds it (asserted below); a v that is taken is an f
//   chain       ends at the anchor e with the greatest f; equal f by the least pq, then the least pt
//   record      aln_chain_record: f(e), count(e), start(e).pq, pq_e + k, start(e).pt, pt_e + k, A, flags.  A == 0: all zero.
//               A > max_pair_seeds: ALN_CHAIN_OVERFLOW in flags, A in seeds (0xFFFFFFFF where it is larger), the rest zero
//   filter      kept iff overflowed, or score >= min_score and min(q_end - q_start, t_end - t_start) >= min_span
//   chunks      aln_wordjoin_cut over the candidates' chained anchors: runs of whole candidates of at most chunk_anchors
#pragma once
#include <stdint.h>

#include "aln_seedjoin_rules.h"
#include "../../include/aligner_hip_seedchain.h"

#define ALN_SEEDCHAIN_MAX_GAP 0x7FFFFFFFu
#define ALN_SEEDCHAIN_MAX_SKEW 0x7FFFFFFFu
#define ALN_SEEDCHAIN_MAX_GAP_SCALE 255u
#define ALN_SEEDCHAIN_PAIR_SEEDS (1u << 16)                // max_pair_seeds == 0
#define ALN_SEEDCHAIN_MAX_PAIR_SEEDS (1u << 20)
#define ALN_SEEDCHAIN_CHUNK_ANCHORS (1u << 24)             // chunk_anchors == 0
#define ALN_SEEDCHAIN_MAX_CHUNK_ANCHORS (1u << 26)

static_assert((int64_t)ALN_SEEDJOIN_MAX_K * ALN_SEEDCHAIN_MAX_PAIR_SEEDS <= 0x7FFFFFFF, "f <= k * 2^20 must fit int32_t");
static_assert(sizeof(aln_seedchain_spec) == 48 && sizeof(aln_chain_record) == 32 && sizeof(aln_seedchain_summary) == 32, "pinned sizes");

// what a spec's two defaults stand for
ALN_HD inline uint32_t aln_seedchain_pair_seeds(const aln_seedchain_spec &sp) { return sp.max_pair_seeds ? sp.max_pair_seeds : ALN_SEEDCHAIN_PAIR_SEEDS; }
ALN_HD inline uint32_t aln_seedchain_chunk_anchors(const aln_seedchain_spec &sp) { return sp.chunk_anchors ? sp.chunk_anchors : ALN_SEEDCHAIN_CHUNK_ANCHORS; }

// 0 if the spec's own fields are in range (k and alphabet are held against the built index by the host), else which refusal:
//   1 max_gap  2 max_skew  3 gap_scale  4 max_pair_seeds  5 chunk_anchors  6 flags / reserved  7 max_pair_seeds above chunk_anchors
ALN_HD inline uint32_t aln_seedchain_spec_refusal(const aln_seedchain_spec &sp)
{
    if (sp.max_gap < 1u || sp.max_gap > ALN_SEEDCHAIN_MAX_GAP) return 1;
    if (sp.max_skew > ALN_SEEDCHAIN_MAX_SKEW) return 2;
    if (sp.gap_scale > ALN_SEEDCHAIN_MAX_GAP_SCALE) return 3;
    if (sp.max_pair_seeds > ALN_SEEDCHAIN_MAX_PAIR_SEEDS) return 4;
    if (sp.chunk_anchors > ALN_SEEDCHAIN_MAX_CHUNK_ANCHORS) return 5;
    if (sp.flags != 0u || sp.reserved[0] != 0u || sp.reserved[1] != 0u || sp.reserved[2] != 0u) return 6;
    if (aln_seedchain_pair_seeds(sp) > aln_seedchain_chunk_anchors(sp)) return 7;
    return 0;
}

// an anchor as one number, pq << 32 | pt: ascending numbers are ascending by (pq, pt)
ALN_HD inline uint64_t aln_seedchain_anchor(uint32_t pq, uint32_t pt) { return (uint64_t)pq << 32 | pt; }
ALN_HD inline uint32_t aln_seedchain_pq(uint64_t anchor) { return (uint32_t)(anchor >> 32); }
ALN_HD inline uint32_t aln_seedchain_pt(uint64_t anchor) { return (uint32_t)anchor; }

// the anchors a pair chains: A, or none where it overflows; and A as a record holds it
ALN_HD inline uint64_t aln_seedchain_chained(uint64_t a, uint32_t max_pair_seeds) { return a > max_pair_seeds ? 0u : a; }
ALN_HD inline uint32_t aln_seedchain_seeds(uint64_t a) { return a > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)a; }

// dd of the rule, in 64 bits
ALN_HD inline int64_t aln_seedchain_drift(uint64_t j, uint64_t i)
{
    return ((int64_t)aln_seedchain_pt(i) - (int64_t)aln_seedchain_pt(j)) - ((int64_t)aln_seedchain_pq(i) - (int64_t)aln_seedchain_pq(j));
}

// j in Pred(i)
ALN_HD inline bool aln_seedchain_pred(uint64_t j, uint64_t i, uint32_t max_gap, uint32_t max_skew)
{
    const uint32_t pq_j = aln_seedchain_pq(j), pt_j = aln_seedchain_pt(j), pq_i = aln_seedchain_pq(i), pt_i = aln_seedchain_pt(i);
    if (pq_j >= pq_i || pt_j >= pt_i) return false;
    if (pq_i - pq_j > max_gap || pt_i - pt_j > max_gap) return false;
    const int64_t dd = aln_seedchain_drift(j, i);
    return (dd < 0 ? -dd : dd) <= (int64_t)max_skew;
}

// v(j, i) for a j in Pred(i) whose f is f_j
ALN_HD inline int64_t aln_seedchain_value(int32_t f_j, uint64_t j, uint64_t i, uint32_t k, uint32_t gap_scale)
{
    const uint32_t dq = aln_seedchain_pq(i) - aln_seedchain_pq(j), dt = aln_seedchain_pt(i) - aln_seedchain_pt(j);
    const uint32_t least = dq < dt ? dq : dt;
    const int64_t gain = least < k ? least : k;
    const int64_t dd = aln_seedchain_drift(j, i);
    const int64_t cost = (int64_t)(((uint64_t)(dd < 0 ? -dd : dd) * gap_scale) >> 4);
    return (int64_t)f_j + gain - cost;
}

// One anchor's link so far: taken iff v > k.  The empty link is {k, 0, 0}: any v > k beats it, whatever its anchor
struct aln_seedchain_link {
    int64_t v;
    uint64_t anchor;               // the predecessor, pq << 32 | pt
    uint64_t at;                   // where it is stored
};
ALN_HD inline aln_seedchain_link aln_seedchain_no_link(uint32_t k) { return aln_seedchain_link{(int64_t)k, 0u, 0u}; }
// does a beat b as a predecessor: the greater v; equal v by the greater pq, then the greater pt -- the greater anchor number.  Two
// anchors of a pair never share (pq, pt), so among taken links the order is total
ALN_HD inline bool aln_seedchain_link_beats(const aln_seedchain_link &a, const aln_seedchain_link &b)
{
    return a.v > b.v || (a.v == b.v && a.anchor > b.anchor);
}

// One anchor as the chain's end so far.  The empty end has f = 0, below every anchor's f >= k >= 1
struct aln_seedchain_end {
    int32_t f;
    uint64_t anchor;
    uint64_t at;
};
ALN_HD inline aln_seedchain_end aln_seedchain_no_end() { return aln_seedchain_end{0, ~0ull, 0u}; }
// does a beat b as the end: the greater f; equal f by the least pq, then the least pt -- the lesser anchor number
ALN_HD inline bool aln_seedchain_end_beats(const aln_seedchain_end &a, const aln_seedchain_end &b)
{
    return a.f > b.f || (a.f == b.f && a.anchor < b.anchor);
}

// what chaining keeps per anchor, 16 bytes beside the anchor's 8
struct aln_seedchain_state {
    int32_t f;
    uint32_t count;
    uint64_t start;                // pq << 32 | pt
};
static_assert(sizeof(aln_seedchain_state) == 16, "16 bytes per anchor");

// the state of anchor i given its best link
ALN_HD inline aln_seedchain_state aln_seedchain_settle(uint64_t i, const aln_seedchain_link &best, const aln_seedchain_state *state, uint32_t k)
{
    if (best.v > (int64_t)k) return aln_seedchain_state{(int32_t)best.v, state[best.at].count + 1u, state[best.at].start};
    return aln_seedchain_state{(int32_t)k, 1u, i};
}

ALN_HD inline aln_chain_record aln_seedchain_record_none(uint64_t a, uint32_t max_pair_seeds)      // A == 0, or overflow
{
    aln_chain_record r = {0, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (a > max_pair_seeds) { r.seeds = aln_seedchain_seeds(a); r.flags = ALN_CHAIN_OVERFLOW; }
    return r;
}
ALN_HD inline aln_chain_record aln_seedchain_record(const aln_seedchain_end &e, const aln_seedchain_state &s, uint64_t a, uint32_t k)
{
    aln_chain_record r;
    r.score = s.f; r.anchors = s.count;
    r.q_start = aln_seedchain_pq(s.start); r.q_end = aln_seedchain_pq(e.anchor) + k;
    r.t_start = aln_seedchain_pt(s.start); r.t_end = aln_seedchain_pt(e.anchor) + k;
    r.seeds = aln_seedchain_seeds(a); r.flags = 0u;
    return r;
}

ALN_HD inline bool aln_seedchain_keep(const aln_chain_record &r, int32_t min_score, uint32_t min_span)
{
    if (r.flags & ALN_CHAIN_OVERFLOW) return true;
    const uint32_t sq = r.q_end - r.q_start, st = r.t_end - r.t_start;
    return r.score >= min_score && (sq < st ? sq : st) >= min_span;
}

// Where the predecessors of stored anchor i can lie, anchors stored ascending in pq (those of equal pq in any order): from the first
// stored anchor with pq >= pq_i - G to before the first with pq == pq_i, two bisections over the i anchors in front of it.  Every
// member of Pred(i) is inside (pq_j < pq_i, pq_i - pq_j <= G); aln_seedchain_pred decides about each one
ALN_HD inline void aln_seedchain_window(const uint64_t *anchors, uint64_t i, uint32_t max_gap, uint64_t *lo, uint64_t *hi)
{
    const uint32_t pq = aln_seedchain_pq(anchors[i]);
    *lo = aln_postings_lower_bound(anchors, i, aln_seedchain_anchor(pq > max_gap ? pq - max_gap : 0u, 0u));
    *hi = aln_postings_lower_bound(anchors, i, aln_seedchain_anchor(pq, 0u));
}

// One pair's chain as one loop (the CPU driver's; the kernel gives a wave to the pair and strides its lanes over j).  anchors: the A
// anchors ascending in pq, those of equal pq in ANY order; state: A entries of scratch
ALN_HD inline aln_chain_record aln_seedchain_pair(const uint64_t *anchors, uint64_t a, const aln_seedchain_spec &sp, aln_seedchain_state *state)
{
    const uint32_t cap = aln_seedchain_pair_seeds(sp);
    if (a == 0u || a > cap) return aln_seedchain_record_none(a, cap);
    aln_seedchain_end end = aln_seedchain_no_end();
    for (uint64_t i = 0; i < a; ++i) {
        aln_seedchain_link best = aln_seedchain_no_link(sp.k);
        uint64_t lo, hi;
        aln_seedchain_window(anchors, i, sp.max_gap, &lo, &hi);
        for (uint64_t j = lo; j < hi; ++j) {
            if (!aln_seedchain_pred(anchors[j], anchors[i], sp.max_gap, sp.max_skew)) continue;
            const aln_seedchain_link l = {aln_seedchain_value(state[j].f, anchors[j], anchors[i], sp.k, sp.gap_scale), anchors[j], j};
            if (l.v > (int64_t)sp.k && aln_seedchain_link_beats(l, best)) best = l;
        }
        state[i] = aln_seedchain_settle(anchors[i], best, state, sp.k);
        const aln_seedchain_end e = {state[i].f, anchors[i], i};
        if (aln_seedchain_end_beats(e, end)) end = e;
    }
    return aln_seedchain_record(end, state[end.at], a, sp.k);
}
