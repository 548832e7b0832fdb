// aln_seedchain.hip -- device side of the seed chains of a resident sequence set's candidate list (aln_seqset_candidate_chains /
// _chain_filter, include/aligner_hip_seedchain.h; the rule is aln_seedchain_rules.h).  P is the seed index of aln_seedjoin.hip: every
// occurrence's key word << 32 | seq ascending, its position beside it.
//
//   count      one wave per candidate (q, t); its lanes take the window starts pq of q, 64 a round.  The word at (q, pq) by
//              aln_prefilter_word; the word's run in P by two bisections, a run longer than max_occ dropped; the (word, t) sub-run by
//              two more: its length is this pq's anchors.  A wave sum over all rounds is A.  Lane 0 leaves A, what the pair chains
//              (none where it overflows) and the record of a pair that is not chained
//   offsets    aln_select.h's offsets step over the chained counts: 64-bit anchor offsets (the host cuts the list into runs of whole
//              candidates of at most chunk_anchors by aln_wordjoin_cut and hands a chunk its first offset)
//   expand     as count; a wave prefix over a round's lengths places each pq's anchors, ascending in pq, the pt of one pq in the
//              order P holds them.  8 bytes an anchor
//   chain      one wave per candidate, its anchors taken in stored order.  For anchor i the window of aln_seedchain_window; the lanes
//              stride over it, each keeps its best link, a wave reduction under the rule's tie order picks j*, lane 0 settles i (16
//              bytes of state beside the anchor).  A second strided pass and reduction find the end.  The block is that one wave, so
//              the barrier behind lane 0's store is the wave's own and what it stored is read back by every lane after it
//   filter     aln_select.h with Keep = the rule's filter over the records, Emit = the entry's place, its pair number and its record
//
// Every index is compared with the size of what it indexes, in 64 bits, before it is used; every loop is a bisection (at most 64
// trips) or runs to a count the host passed or the set's own tables hold.  Every store is a plain C++ store of a thread; the only
// atomics are integer atomicAdd on the error counter.  A * (window / 64) dependent rounds per candidate is the chain's known cost:
// max_occ and max_pair_seeds are the remedies.
#include "aln_postings.h"
#include "aln_launch.h"
#include "aln_seedchain_rules.h"
#include "aln_select.h"

constexpr uint32_t ALN_SC_WAVE = 64u;
constexpr uint32_t ALN_SC_COUNT_THREADS = 256u;            // count and expand: four candidates a block

// what count and expand know of the set and the index
struct ScIndex {
    const uint8_t *seqs;
    const uint64_t *seq_off;
    const uint32_t *seq_len;
    uint64_t n_seqs, total;                                // records, residues
    const uint64_t *keys;
    const uint32_t *pos;
    uint64_t n;                                            // occurrences of P
    uint32_t k, alphabet, max_occ;
};

// the sub-run [*a, *z) of P that holds the anchors of window start pq of record q against record t; false: none
__device__ __forceinline__ bool sc_sub_run(const ScIndex &x, uint64_t q, uint64_t t, uint64_t pq, uint64_t *a, uint64_t *z)
{
    const uint64_t len = x.seq_len[q], at = x.seq_off[q] + pq;
    if (pq >= len || pq + x.k > len || at + x.k > x.total) return false;
    uint32_t w;
    if (!aln_prefilter_word(x.seqs + at, x.k, x.alphabet, &w)) return false;
    const uint64_t word = (uint64_t)w << 32;
    if (x.max_occ) {
        const uint64_t ra = aln_postings_lower_bound(x.keys, x.n, word), rz = aln_postings_upper_bound(x.keys, x.n, word | 0xFFFFFFFFull);
        if (rz > ra && rz - ra > x.max_occ) return false;
    }
    *a = aln_postings_lower_bound(x.keys, x.n, word | t);
    *z = aln_postings_upper_bound(x.keys, x.n, word | t);
    return *z > *a && *z <= x.n;
}

__device__ __forceinline__ uint64_t sc_wave_sum(uint64_t v)
{
    for (uint32_t o = ALN_SC_WAVE / 2u; o; o >>= 1) v += __shfl_xor(v, o, ALN_SC_WAVE);
    return v;
}
// the lane's exclusive prefix of v over the wave, and the wave's sum
__device__ __forceinline__ uint64_t sc_wave_exclusive(uint64_t v, uint32_t lane, uint64_t *sum)
{
    uint64_t incl = v;
    for (uint32_t o = 1; o < ALN_SC_WAVE; o <<= 1) {
        const uint64_t up = __shfl_up(incl, o, ALN_SC_WAVE);
        if (lane >= o) incl += up;
    }
    *sum = __shfl(incl, ALN_SC_WAVE - 1u, ALN_SC_WAVE);
    return incl - v;
}

// ---- A of candidates 0 .. n - 1 (cand_q / cand_t: their records), what each chains, and the records of those that chain nothing
__global__ __launch_bounds__(256) void aln_seedchain_count_kernel(ScIndex x, const uint32_t *cand_q, const uint32_t *cand_t, uint64_t n,
                                                                  uint32_t max_pair_seeds, uint32_t *seeds, uint32_t *chained,
                                                                  aln_chain_record *records, uint32_t *errors)
{
    const uint32_t lane = threadIdx.x % ALN_SC_WAVE;
    const uint64_t c = (uint64_t)blockIdx.x * (ALN_SC_COUNT_THREADS / ALN_SC_WAVE) + threadIdx.x / ALN_SC_WAVE;
    if (c >= n) return;
    const uint64_t q = cand_q[c], t = cand_t[c];
    uint64_t mine = 0;
    if (q >= x.n_seqs || t >= x.n_seqs) { if (lane == 0) atomicAdd(errors, 1u); }
    else {
        const uint64_t windows = aln_prefilter_windows(x.seq_len[q], x.k);
        for (uint64_t pq = lane; pq < windows; pq += ALN_SC_WAVE) {
            uint64_t a, z;
            if (sc_sub_run(x, q, t, pq, &a, &z)) mine += z - a;
        }
    }
    const uint64_t all = sc_wave_sum(mine);
    if (lane == 0) {
        seeds[c] = aln_seedchain_seeds(all);
        chained[c] = (uint32_t)aln_seedchain_chained(all, max_pair_seeds);      // (at most max_pair_seeds <= 2^20)
        records[c] = aln_seedchain_record_none(all, max_pair_seeds);
    }
}

// ---- the anchors of candidates c0 .. c0 + m - 1 into out[0 .. room): candidate c's at offsets[c] - base, chained[c] of them
__global__ __launch_bounds__(256) void aln_seedchain_expand_kernel(ScIndex x, const uint32_t *cand_q, const uint32_t *cand_t, uint64_t c0, uint64_t m,
                                                                   const uint32_t *chained, const uint64_t *offsets, uint64_t base, uint64_t room,
                                                                   uint64_t *out, uint32_t *errors)
{
    const uint32_t lane = threadIdx.x % ALN_SC_WAVE;
    const uint64_t r = (uint64_t)blockIdx.x * (ALN_SC_COUNT_THREADS / ALN_SC_WAVE) + threadIdx.x / ALN_SC_WAVE;
    if (r >= m) return;
    const uint64_t c = c0 + r, want = chained[c];
    if (!want) return;
    const uint64_t q = cand_q[c], t = cand_t[c];
    if (q >= x.n_seqs || t >= x.n_seqs || offsets[c] < base || offsets[c] - base > room || want > room - (offsets[c] - base)) {
        if (lane == 0) atomicAdd(errors, 1u);
        return;
    }
    uint64_t *mine = out + (offsets[c] - base);
    const uint64_t windows = aln_prefilter_windows(x.seq_len[q], x.k);
    uint64_t done = 0;                                     // the anchors of the rounds before: the same in every lane
    for (uint64_t round = 0; round < windows; round += ALN_SC_WAVE) {
        const uint64_t pq = round + lane;
        uint64_t a = 0, z = 0;
        if (pq >= windows || !sc_sub_run(x, q, t, pq, &a, &z)) a = z = 0;
        uint64_t sum;
        const uint64_t at = done + sc_wave_exclusive(z - a, lane, &sum);
        if (z - a > want || at > want - (z - a) || pq >= 0x80000000ull) { if (z > a) atomicAdd(errors, 1u); }
        else
            for (uint64_t j = 0; j < z - a; ++j) {
                const uint32_t pt = x.pos[a + j];
                if (pt >= 0x80000000u) atomicAdd(errors, 1u);          // (never on a sound index: the host answers ALN_ERR_DEVICE)
                else mine[at + j] = aln_seedchain_anchor((uint32_t)pq, pt);
            }
        done += sum;
    }
    if (lane == 0 && done != want) atomicAdd(errors, 1u);
}

// ---- the chains of candidates c0 .. c0 + m - 1 of a chunk; anchors / state: the chunk's, candidate c's at offsets[c] - base
__global__ __launch_bounds__(64) void aln_seedchain_chain_kernel(const uint64_t *anchors, aln_seedchain_state *state, uint64_t c0, uint64_t m,
                                                                 const uint32_t *seeds, const uint32_t *chained, const uint64_t *offsets, uint64_t base,
                                                                 uint64_t room, aln_seedchain_spec sp, aln_chain_record *records, uint32_t *errors)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t r = blockIdx.x;
    if (r >= m) return;
    const uint64_t c = c0 + r, a = chained[c];
    if (!a) return;                                        // (the count kernel left its record)
    if (offsets[c] < base || offsets[c] - base > room || a > room - (offsets[c] - base)) {
        if (lane == 0) atomicAdd(errors, 1u);
        return;
    }
    const uint64_t *anc = anchors + (offsets[c] - base);
    aln_seedchain_state *st = state + (offsets[c] - base);
    uint64_t lo = 0, hi = 0, before = ~0ull;               // the window of the anchor before, whose pq was `before` >> 32
    for (uint64_t i = 0; i < a; ++i) {
        const uint64_t me = anc[i];
        if (i && aln_seedchain_pq(before) > aln_seedchain_pq(me)) { if (lane == 0) atomicAdd(errors, 1u); return; }      // not ascending in pq
        if (!i || aln_seedchain_pq(before) != aln_seedchain_pq(me)) aln_seedchain_window(anc, i, sp.max_gap, &lo, &hi);  // (equal pq: the same window)
        before = me;
        aln_seedchain_link best = aln_seedchain_no_link(sp.k);
        for (uint64_t j = lo + lane; j < hi; j += ALN_SC_WAVE) {
            const uint64_t other = anc[j];
            if (!aln_seedchain_pred(other, me, sp.max_gap, sp.max_skew)) continue;
            const aln_seedchain_link l = {aln_seedchain_value(st[j].f, other, me, sp.k, sp.gap_scale), other, j};
            if (l.v > (int64_t)sp.k && aln_seedchain_link_beats(l, best)) best = l;
        }
        for (uint32_t o = ALN_SC_WAVE / 2u; o; o >>= 1) {
            const aln_seedchain_link l = {(int64_t)__shfl_xor((long long)best.v, o, ALN_SC_WAVE), (uint64_t)__shfl_xor((unsigned long long)best.anchor, o, ALN_SC_WAVE),
                                          (uint64_t)__shfl_xor((unsigned long long)best.at, o, ALN_SC_WAVE)};
            if (l.v > (int64_t)sp.k && aln_seedchain_link_beats(l, best)) best = l;
        }
        if (lane == 0) st[i] = aln_seedchain_settle(me, best.at < i ? best : aln_seedchain_no_link(sp.k), st, sp.k);
        __syncthreads();                                   // one wave: its own barrier, and st[i] is visible to every lane behind it
    }
    aln_seedchain_end end = aln_seedchain_no_end();
    for (uint64_t i = lane; i < a; i += ALN_SC_WAVE) {
        const aln_seedchain_end e = {st[i].f, anc[i], i};
        if (aln_seedchain_end_beats(e, end)) end = e;
    }
    for (uint32_t o = ALN_SC_WAVE / 2u; o; o >>= 1) {
        const aln_seedchain_end e = {(int32_t)__shfl_xor(end.f, o, ALN_SC_WAVE), (uint64_t)__shfl_xor((unsigned long long)end.anchor, o, ALN_SC_WAVE),
                                     (uint64_t)__shfl_xor((unsigned long long)end.at, o, ALN_SC_WAVE)};
        if (aln_seedchain_end_beats(e, end)) end = e;
    }
    if (lane == 0) {
        if (end.at < a) records[c] = aln_seedchain_record(end, st[end.at], seeds[c], sp.k);
        else atomicAdd(errors, 1u);
    }
}

// ---- the filter: the kept entries' places, pair numbers and records, in list order
struct ScKeep {
    const aln_chain_record *records;
    int32_t min_score;
    uint32_t min_span;
    __device__ bool operator()(uint64_t c) const { return aln_seedchain_keep(records[c], min_score, min_span); }
};
struct ScEmit {
    const aln_chain_record *records;
    const uint64_t *cand_k;
    uint64_t room;
    uint32_t *out_pos;
    uint64_t *out_k;
    aln_chain_record *out_records;
    __device__ void operator()(uint32_t o, uint64_t c) const
    {
        if (o >= room) return;
        out_pos[o] = (uint32_t)c;
        out_k[o] = cand_k[c];
        out_records[o] = records[c];
    }
};

extern "C" int aln_warm_seedchain(void)
{
    hipFuncAttributes a;
    return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&aln_seedchain_chain_kernel));
}

static ScIndex sc_index(const aln_seedchain_index *x, const aln_seedchain_spec *sp)
{
    return ScIndex{x->seqs, x->seq_off, x->seq_len, x->n_seqs, x->total, x->keys, x->pos, x->n, sp->k, sp->alphabet, sp->max_occ};
}

extern "C" void aln_seedchain_launch_count(const aln_seedchain_index *x, const aln_seedchain_spec *sp, const uint32_t *cand_q, const uint32_t *cand_t,
                                           uint64_t n, uint32_t *seeds, uint32_t *chained, uint64_t *offsets, uint64_t *total,
                                           aln_chain_record *records, uint32_t *errors, hipStream_t s)
{
    const uint32_t per = ALN_SC_COUNT_THREADS / ALN_SC_WAVE;
    if (n) hipLaunchKernelGGL(aln_seedchain_count_kernel, dim3(blocks_of(n, per)), dim3(ALN_SC_COUNT_THREADS), 0, s, sc_index(x, sp), cand_q, cand_t, n,
                              aln_seedchain_pair_seeds(*sp), seeds, chained, records, errors);
    hipLaunchKernelGGL(aln_select_offsets_kernel<uint64_t>, dim3(1), dim3(ALN_SELECT_THREADS), 0, s, chained, offsets, n, total);
}

extern "C" void aln_seedchain_launch_chunk(const aln_seedchain_index *x, const aln_seedchain_spec *sp, const uint32_t *cand_q, const uint32_t *cand_t,
                                           uint64_t c0, uint64_t m, const uint32_t *seeds, const uint32_t *chained, const uint64_t *offsets,
                                           uint64_t base, uint64_t room, uint64_t *anchors, void *state, aln_chain_record *records, uint32_t *errors,
                                           hipStream_t s)
{
    if (!m || !room) return;
    const uint32_t per = ALN_SC_COUNT_THREADS / ALN_SC_WAVE;
    hipLaunchKernelGGL(aln_seedchain_expand_kernel, dim3(blocks_of(m, per)), dim3(ALN_SC_COUNT_THREADS), 0, s, sc_index(x, sp), cand_q, cand_t, c0, m, chained,
                       offsets, base, room, anchors, errors);
    hipLaunchKernelGGL(aln_seedchain_chain_kernel, dim3((uint32_t)m), dim3(ALN_SC_WAVE), 0, s, anchors, static_cast<aln_seedchain_state *>(state), c0, m, seeds,
                       chained, offsets, base, room, *sp, records, errors);
}

extern "C" void aln_seedchain_launch_filter(const aln_chain_record *records, const uint64_t *cand_k, uint64_t n, int32_t min_score, uint32_t min_span,
                                            uint32_t *tile_count, uint32_t *tile_off, uint32_t *count, uint64_t room, uint32_t *out_pos, uint64_t *out_k,
                                            aln_chain_record *out_records, hipStream_t s)
{
    aln_select_launch(ScKeep{records, min_score, min_span}, ScEmit{records, cand_k, room, out_pos, out_k, out_records}, n, tile_count, tile_off, count, s);
}
