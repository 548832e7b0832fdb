// aln_plan_rules.h -- the batch plan: what aln_host.hip decides about a chunk of pairs before anything is launched.  Plain
// arithmetic on lengths, offsets and the call's facts: no HIP and no getenv, so that a test can compile and run the real rules on a
// machine without a GPU (tests/test_plan_rules_cpu.py).
//
//   AlnPlanCall     the facts of a call that the plan reads; AlnPlanKnobs: the ALN_* settings, parsed by the host
//   Chunk           the plan of one chunk; aln_plan_chunk fills it, step by step in this order:
//     aln_plan_descs           descriptors and residue span
//     aln_big_to_single        the time rule: large pairs to the single-pair route, or shared by the batch kernel's waves
//     aln_plan_routes          per pair: single-pair kernel (aln_single_route_r), one workgroup (aln_wg_route_r) or batch kernel;
//                              direction, string, tag and H layout
//     aln_plan_order           the LPT order of the batch kernel's queue, by aln_pair_cost
//     aln_plan_grid            grid and overlapped walk
//     aln_plan_share           what can be shared; cooperative or lean build (aln_coop_lean_plan); tail, linger, chain grid
//     aln_plan_scratch_lds     scratch stride (aln_scratch_stride) and LDS
//     aln_plan_duo             two short pairs per wave
//   aln_plan_bounds upper bounds of a range of pairs, for slots that are sized once before a pipeline runs
//   aln_make_chunks where a batch call is cut (aln_chunk_target, aln_shuffle_chunk_target, aln_chunk_cells_override)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/aligner_hip.h"
#include "aln_layout_rules.h"

// ---------------------------------------------------------------- what the plan reads
struct AlnPlanCall {
    bool pwm = false, fast = false, is_int = true;
    bool want_h = false, want_tb = true, store_dirs = true;
    bool hazard = false;              // core local with del != ext: a pair may be re-filled (the row-1 hazard)
    bool force_serial = false;
    bool pair_matrices = false;       // one matrix per pair (aln_pairset_run)
    int semantics = 0;                // what the kernels run (PWM runs as ALN_CORE_LOCAL)
    uint32_t rows = 0, cols = 0;
};
// an ALN_* variable with a value: whether it is set, and atoi / strtoull of it
struct AlnKnob {
    bool set = false;
    long long v = 0;
};
struct AlnPlanKnobs {
    AlnKnob single_r;                 // ALN_SINGLE_R: rows per lane of the single-pair route (1, 2, 4, 8; anything else: 2)
    bool no_single = false;           // ALN_NO_SINGLE: nothing goes to the single-pair route
    bool no_coop = false;             // ALN_NO_COOP: no cooperative passes, and large pairs routed as if nothing could be shared
    AlnKnob big_to_single;            // ALN_BIG_TO_SINGLE: overrides the time rule (0: large pairs stay with the batch kernel)
    bool no_wgpipe = false;           // ALN_NO_WGPIPE: no one-workgroup route
    AlnKnob wg_r;                     // ALN_WG_R: rows per lane of the one-workgroup route (1, 2, 4, at most 16 strips)
    AlnKnob tb_overlap;               // ALN_TB_OVERLAP: 0 = no walk beside the fill, n > 0 = the fill grid stops n workgroups short
    bool tb_overlap_any = false;      // ALN_TB_OVERLAP_ANY: the walk beside the fill also below 2e9 cells
    int coop_lean = -1;               // ALN_COOP_LEAN: < 0 unset (aln_coop_lean_plan decides), 0 never lean, > 0 always lean
    AlnKnob coop_tail;                // ALN_COOP_TAIL: pairs from the end of the queue whose first pass is opened
    AlnKnob chain_wgs;                // ALN_CHAIN_WGS: 0 = chains of strips keep three waves per SIMD
    AlnKnob fill_wgs;                 // ALN_FILL_WGS: at most this many fill workgroups (experiments)
    bool no_duo = false;              // ALN_NO_DUO: never two pairs per wave
    bool trace_plan = false;          // ALN_TRACE_PLAN: the host prints what was planned
    bool chunk_cells_set = false;     // ALN_CHUNK_CELLS: the cells a chunk aims at (aln_chunk_cells_override)
    double chunk_cells = 0;
};

// ---------------------------------------------------------------- per chunk: descriptors, routing, layout
struct Chunk {
    size_t first = 0, n = 0;          // pairs [first, first + n) of the call
    std::vector<PairDesc> descs;
    std::vector<uint32_t> order;      // LPT order of the device work queue (pairs of the batch kernel)
    std::vector<uint32_t> single_pairs, single_r;   // pairs routed to the single-pair (one wave per strip) kernel
    std::vector<uint32_t> wg_pairs, wg_r;           // generic kernels: pairs filled by one workgroup each (aln_fill_wgpipe_kernel)
    size_t n_small = 0;
    uint64_t cells = 0, max_cells = 0, dir_bytes = 0, tb_bytes = 0, tag_bytes = 0, hmat_elems = 0;
    uint32_t max_len = 1, grid = 1, zrow_bytes = 0, lds_bytes = 0, prof_stride = 0, tb_waves = 0, single_max_n = 0, cascade_rows = 1;
    uint32_t duo_qo = 0;               // != 0: two short pairs per wave (aln_fill_duo_kernel): u16 entries of one staged query
    uint64_t scratch_stride = 0, granule_bytes = 0, tbmap_entries = 0, granule_stride_max = 0;
    size_t counter_bytes = 256;
    bool overlap = false;             // walk waves beside the fill (in-kernel overlapped traceback)
    // cooperative passes of the fast batch kernel (CoopRec, aln_device.h): hint ring capacities, bytes of the control block
    bool coop = false, coop_linger = false;
    bool coop_lean = false;           // the chunk would share, but so little that the kernel build without the machinery runs it (aln_coop_lean)
    uint32_t coop_tail = 0;
    uint64_t coop_bytes = 0;
    // sequences: either one contiguous span of the caller's buffer, or gathered pair by pair into pinned staging
    bool seq_direct = true;
    uint64_t seq_lo = 0, seq_span = 0;
    // a plan that is planned again keeps its arrays (6.4 MB of descriptors for 100 000 pairs: allocating and faulting them in afresh
    // was 1 of the 2 ms the plan of a 100 000-window call took)
    void reset()
    {
        std::vector<PairDesc> d = std::move(descs);
        std::vector<uint32_t> o = std::move(order), sp = std::move(single_pairs), sr = std::move(single_r), wp = std::move(wg_pairs), wr = std::move(wg_r);
        *this = Chunk();
        d.clear(); o.clear(); sp.clear(); sr.clear(); wp.clear(); wr.clear();
        descs = std::move(d); order = std::move(o); single_pairs = std::move(sp); single_r = std::move(sr); wg_pairs = std::move(wp); wg_r = std::move(wr);
    }
};

// ---------------------------------------------------------------- residue span, strings, tags
// The residues of a range of pairs are one span of the caller's buffer unless the offsets are scattered far beyond what the range
// uses; then they are gathered pair by pair.
struct AlnSeqSpan {
    uint64_t lo = ~0ull, hi = 0, sum = 0;
    void add(uint64_t off, uint64_t len)
    {
        if (!len) return;
        lo = std::min(lo, off); hi = std::max(hi, off + len); sum += len;
    }
    void add_pair(bool pwm, uint64_t q_off, uint64_t q_len, uint64_t t_off, uint64_t t_len)
    {
        if (!pwm) add(q_off, q_len);
        add(t_off, t_len);
    }
    bool empty() const { return lo == ~0ull; }
    uint64_t extent() const { return empty() ? 0 : hi - lo; }
    bool direct() const { return extent() <= 2 * sum + 65536; }
    uint64_t bytes() const { return direct() ? extent() : sum; }
};
// strings: cumulative 2 * cap per pair (PWM: 5 * cap, 4-aligned) -- the layout aln_align_batch documents for tb_buf; cap = N + M + 2
inline uint64_t aln_tb_bytes(bool pwm, uint64_t cap) { return pwm ? ((5ull * cap + 3) & ~3ull) : 2ull * cap; }
inline uint64_t aln_tag_bytes(uint64_t cap) { return (cap + 3) & ~3ull; }

// Step 1: the descriptors of the chunk's pairs (lengths, status, residue offsets) and its residue span
inline void aln_plan_descs(const AlnPlanCall &c, const uint64_t *q_off, const uint64_t *q_len, const uint64_t *t_off, const uint64_t *t_len,
                           size_t first, size_t n, Chunk &k)
{
    k.first = first; k.n = n;
    k.descs.assign(n, PairDesc{});
    const bool pwm = c.pwm;
    AlnSeqSpan span;
    for (size_t i = 0; i < n; ++i) {
        const size_t g = first + i;
        PairDesc &d = k.descs[i];
        d.N = pwm ? c.cols : (uint32_t)q_len[g];                               // PWM: the columns are the PWM positions
        d.M = (uint32_t)t_len[g];
        d.status = ALN_OK;
        if (d.N == 0 || d.M == 0) d.status = (pwm && d.N != 0) ? ALN_PRE_EMPTY_OK : ALN_ERR_EMPTY_SEQUENCE;   // the reference panics
        span.add_pair(pwm, q_off[g], q_len[g], t_off[g], t_len[g]);
    }
    const uint64_t seq_lo = span.empty() ? 0 : span.lo;
    k.seq_direct = span.direct();
    k.seq_lo = seq_lo;
    k.seq_span = span.bytes();
    uint64_t gpos = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t g = first + i;
        PairDesc &d = k.descs[i];
        if (k.seq_direct) { d.q_off = pwm ? 0 : q_off[g] - (q_len[g] ? seq_lo : q_off[g]); d.t_off = t_len[g] ? t_off[g] - seq_lo : 0; }
        else { d.q_off = gpos; gpos += pwm ? 0 : q_len[g]; d.t_off = gpos; gpos += t_len[g]; }
    }
}

// ---------------------------------------------------------------- routing
// A pair goes to the single-pair kernel (one wave per strip, strips pipelined across CUs) when it is large, or when the chunk is
// too small to fill the chip with one wave per pair -- unless the chunk holds so many such pairs that the batch kernel, whose waves
// share the strips of a pair (cooperative passes), is through with all of them sooner than the single-pair route, which takes them
// one after the other (aln_big_to_single).
inline bool aln_big_pair(const PairDesc &d, size_t n)
{
    const uint64_t pc = (uint64_t)d.N * d.M;
    return d.N >= 64 && d.M >= 128 && (pc >= (1ull << 24) || (n <= 16 && pc >= (1ull << 18)));
}
inline bool aln_coop_on(const AlnPlanCall &c, const AlnPlanKnobs &kn) { return c.fast && !kn.no_coop; }

// Step 2, the time rule.  Estimates (measured rates): the single-pair route fills at ~60 GCUPS plus ~0.2 ms of launches and
// traceback per pair; in the batch kernel a wave fills at ~0.85 GCUPS with the chip full (2.6 TCUPS at most), and the pipeline of
// a pair's strips takes (N + 63 + 170 (strips - 1)) steps of ~0.55 us.
inline bool aln_big_to_single(uint32_t cus, const AlnPlanCall &c, const AlnPlanKnobs &kn, const Chunk &k)
{
    if (!aln_coop_on(c, kn) || c.pwm || kn.no_single) return true;
    const size_t n = k.n;
    double t_single = 0, cells_all = 0, cells_small = 0, strips_all = 0, strips_small = 0, lat_all = 0, lat_small = 0;
    size_t n_big = 0;
    for (size_t i = 0; i < n; ++i) {
        const PairDesc &d = k.descs[i];
        if (d.status != ALN_OK) continue;
        const double pc = (double)d.N * d.M, st = (double)aln_num_strips(d.M);
        const double lat = ((double)d.N + 63.0 + 170.0 * (st - 1.0)) * 0.55e-6;
        cells_all += pc; strips_all += st; lat_all = std::max(lat_all, lat);
        if (aln_big_pair(d, n)) { t_single += pc / 60e9 + 0.2e-3; ++n_big; }
        else { cells_small += pc; strips_small += st; lat_small = std::max(lat_small, lat); }
    }
    const double waves = (double)cus * 12.0;
    auto t_batch = [&](double cells, double strips, double lat) {
        if (cells <= 0) return 0.0;
        return std::max(std::max(cells / 2.6e12, lat), cells / (std::min(strips, waves) * 0.85e9));
    };
    bool big_to_single = true;
    if (n_big) big_to_single = t_single + t_batch(cells_small, strips_small, lat_small) <= t_batch(cells_all, strips_all, lat_all);
    if (kn.big_to_single.set) big_to_single = kn.big_to_single.v != 0;
    return big_to_single;
}

inline uint32_t aln_uniform_strips(uint32_t M, uint32_t R) { return (M + 64 * R - 1) / (64 * R); }

// Rows per lane of a pair on the single-pair route; 0 = the route refuses it.
inline uint32_t aln_single_route_r(const AlnPlanCall &c, const AlnPlanKnobs &kn, const PairDesc &d)
{
    // rows per lane: two above ~2500 rows (measured, fill + traceback: 3000 x 3000 0.59 ms against 0.62 with one, 4000 x 4000
    // 0.72 against 0.76; below, the traceback's longer strips cost more than the fill gains)
    uint32_t R = kn.single_r.set ? (uint32_t)(int)kn.single_r.v : (d.M > 2560 ? 2u : 1u);
    if (R != 1 && R != 2 && R != 4 && R != 8) R = 2;
    while (aln_uniform_strips(d.M, R) > 4096 && R < 8) R *= 2;      // keep every strip's wave resident
    if (aln_uniform_strips(d.M, R) > 4096) return 0;
    // LDS: the whole query's profile offsets are staged (2 B per column) beside S and the waves' profiles; a workgroup may
    // opt in to all 160 KiB of a CU (one wave per workgroup beyond ~43 000 columns, four below: aln_single_waves), which
    // carries the route to ~77 000 columns.  Longer pairs take the batch kernel (one wave, slow but exact).
    if (d.N > 100000u || aln_single_lds_bytes(c.rows, c.cols, R, d.N, 1) > 159u * 1024u) return 0;
    return R;
}

// Generic kernels (real-valued matrix, or an integer one outside the fast path's limits): a chunk of at most four pairs (their
// launches run one after the other; a larger chunk is better off with one wave per pair, all at once) gives each pair a whole
// workgroup, one wave per 64 R-row strip (<= 16 strips), instead of one wave -- the call HeuristicAligner makes once per iteration
// (heuristic/mod.rs:58-77).  Also with the H dump (AlignmentResult.alignment_matrix) and for PWM scoring (HeuristicPWMAligner).
// Rows per lane of a pair on that route; 0 = not on it.
inline uint32_t aln_wg_route_r(const AlnPlanCall &c, const AlnPlanKnobs &kn, const PairDesc &d, size_t n)
{
    const uint64_t pc = (uint64_t)d.N * d.M;
    if (!((!c.fast || c.want_h) && !c.pair_matrices && !c.force_serial && !kn.no_wgpipe && n <= 4 && pc >= (1ull << 14) && d.N >= 16 &&
          d.N <= 8192 && d.M >= 65 && d.M <= 2048))
        return 0;
    // rows per lane: about eight strips = two waves per SIMD of the one CU (measured, 1000 x 1000 f64: R = 1 1.42 ms,
    // R = 2 1.26, R = 4 1.28; 330 x 300: 0.43 / 0.43 / 0.50)
    uint32_t R = d.M > 1024 ? 4u : d.M > 512 ? 2u : 1u;
    if (kn.wg_r.set) { const uint32_t v = (uint32_t)(int)kn.wg_r.v; if ((v == 1 || v == 2 || v == 4) && aln_uniform_strips(d.M, v) <= 16) R = v; }
    return aln_wg_lds_bytes(c.rows, c.cols, c.is_int ? 4u : 8u, aln_uniform_strips(d.M, R), d.N) <= 64u * 1024u ? R : 0;
}

// Step 3: every pair's route, and with it the HBM layout of directions, strings, tags and the H dump
inline void aln_plan_routes(const AlnPlanCall &c, const AlnPlanKnobs &kn, bool big_to_single, Chunk &k)
{
    const size_t n = k.n;
    uint64_t dir_total = 0, tb_total = 0, tag_total = 0, hm_total = 0, cells = 0;
    uint32_t max_len = 1;
    for (size_t i = 0; i < n; ++i) {
        PairDesc &d = k.descs[i];
        const uint64_t cap = (uint64_t)d.N + d.M + 2;
        if (c.store_dirs) {
            d.tb_off = tb_total;
            tb_total += aln_tb_bytes(c.pwm, cap);
            d.tag_off = tag_total;
            tag_total += aln_tag_bytes(cap);
        }
        if (d.status != ALN_OK) continue;
        cells += (uint64_t)d.N * d.M;
        max_len = std::max(max_len, std::max(d.N, d.M));
        const bool single_wanted = c.fast && !c.pwm && !kn.no_single && aln_big_pair(d, n) && (big_to_single || aln_num_strips(d.M) > ALN_COOP_MAX_NS);
        const uint32_t single_R = single_wanted ? aln_single_route_r(c, kn, d) : 0u;
        const uint32_t wg_R = single_R ? 0u : aln_wg_route_r(c, kn, d, n);
        uint64_t dbytes = aln_dir_bytes(d.N, d.M);
        if (const uint32_t R = single_R ? single_R : wg_R) {        // both routes: uniform strips, walked through exit maps
            const uint32_t ns = aln_uniform_strips(d.M, R);
            dbytes = std::max<uint64_t>(dbytes, (uint64_t)ns * aln_uniform_strip_bytes(d.N, R));
            k.tbmap_entries = std::max<uint64_t>(k.tbmap_entries, (uint64_t)ns * (d.N + 1) + ns + 64);
            if (single_R) {
                k.single_pairs.push_back((uint32_t)i);
                k.single_r.push_back(R);
                const uint64_t gstride = ((uint64_t)d.N + 64 + 63) & ~63ull;
                k.granule_stride_max = std::max(k.granule_stride_max, gstride);
                k.granule_bytes = std::max<uint64_t>(k.granule_bytes, std::max<uint64_t>((uint64_t)ns * gstride * 4, 4ull * (d.M + 2)));
                k.single_max_n = std::max(k.single_max_n, std::max(d.N, ns));
            } else {
                k.wg_pairs.push_back((uint32_t)i);
                k.wg_r.push_back(R);
            }
        }
        d.dir_off = dir_total;
        if (c.store_dirs) dir_total += dbytes;
        if (c.want_h) { d.h_off = hm_total; hm_total += (uint64_t)(d.N + 1) * (d.M + 1); }
    }
    k.cells = cells; k.max_len = max_len;
    k.dir_bytes = dir_total; k.tb_bytes = tb_total; k.tag_bytes = tag_total; k.hmat_elems = hm_total;
}

// ---------------------------------------------------------------- the queue of the batch kernel
// The strips of a pair in the skewed layout: f(R, L) per strip -- rows per lane and busy lanes; a full strip has R = ALN_FULL_R, the
// last one picks its R by its rows (aln_pick_r).  f returns false to stop the walk.
template <class F> inline void aln_strip_walk(uint32_t M, F f)
{
    const uint32_t ns = aln_num_strips(M);
    for (uint32_t st = 0; st < ns; ++st) {
        const uint32_t rows = std::min<uint32_t>(M - st * ALN_STRIP_ROWS, ALN_STRIP_ROWS);
        const uint32_t R = st + 1 == ns ? (uint32_t)aln_pick_r(rows) : (uint32_t)ALN_FULL_R;
        if (!f(R, (rows + R - 1) / R)) return;
    }
}
// LPT order: longest pairs first into the device work queue.  "Longest" = the time one wave needs, not the cells: a strip of
// R rows per lane takes N + lanes - 1 steps of about 12 + 10.5 R instructions, so a 1900 x 270 pair (one strip of 5 rows per
// lane) keeps its wave as long as a 1000 x 1000 pair with twice the cells -- ordered by cells it was taken when the queue was
// almost dry and ended the 8-way shard's fill 0.9 ms after everybody else (tools/tail_timeline.py).
inline uint64_t aln_pair_cost(const PairDesc &d)
{
    if (d.status != ALN_OK) return 0;
    uint64_t cost = 0;
    aln_strip_walk(d.M, [&](uint32_t R, uint32_t L) {
        cost += (uint64_t)(d.N + L - 1) * (24u + 21u * R);
        return cost < (1ull << 40);
    });
    return std::min<uint64_t>(cost, (1ull << 40) - 1);
}
// bytes the fill kernel actually stores for a pair in the skewed layout: per strip, ceil(steps / SPB) blocks of 256 B
inline uint64_t aln_pair_stored_dir_bytes(const PairDesc &d)
{
    if (d.status != ALN_OK) return 0;
    uint64_t total = 0;
    aln_strip_walk(d.M, [&](uint32_t R, uint32_t L) {
        total += (uint64_t)aln_strip_blocks(d.N + L - 1, aln_spb(R)) * 256u;
        return true;
    });
    return total;
}

// Step 4: the queue = the pairs no other route took, in LPT order (equal costs keep the index order).  Returns the sum of the
// queue's costs (aln_coop_lean_plan).
inline double aln_plan_order(Chunk &k)
{
    const size_t n = k.n;
    k.order.clear();
    k.order.reserve(n);
    {
        std::vector<char> is_single(n, 0);
        for (uint32_t i : k.single_pairs) is_single[i] = 1;
        for (uint32_t i : k.wg_pairs) is_single[i] = 1;
        for (size_t i = 0; i < n; ++i) if (!is_single[i]) k.order.push_back((uint32_t)i);
    }
    k.n_small = k.order.size();
    double cost_sum = 0;
    if (n < (1u << 24)) {
        // sort keys packed in one u64: cost descending, then index ascending (a stable order without a stable_sort)
        std::vector<uint64_t> key(k.n_small);
        for (size_t j = 0; j < k.n_small; ++j) {
            const uint64_t pc = aln_pair_cost(k.descs[k.order[j]]);
            cost_sum += (double)pc;
            key[j] = ((~pc & ((1ull << 40) - 1)) << 24) | k.order[j];
        }
        // (equal pairs -- PWM windows, read pairs -- arrive sorted: the test costs one pass, the sort was 1 of the 1.7 ms the
        // plan of 100 000 windows took)
        if (!std::is_sorted(key.begin(), key.end())) {
            // LSD radix sort on the bits of the cost that vary, 11 at a time (stable: equal costs keep the index order the keys
            // were built in); std::sort was 0.35 of the 0.7 ms the plan of 12 500 pairs took
            uint64_t lo = ~0ull, hi = 0;
            for (uint64_t v : key) { lo = std::min(lo, v >> 24); hi = std::max(hi, v >> 24); }
            const uint64_t range = hi - lo;                      // sort by (v >> 24) - lo
            std::vector<uint64_t> tmp(key.size());
            uint64_t *src = key.data(), *dst = tmp.data();
            for (uint32_t shift = 0; shift < 40 && (range >> shift) != 0; shift += 11) {
                uint32_t cnt[2049] = {0};
                for (size_t j = 0; j < key.size(); ++j) ++cnt[((((src[j] >> 24) - lo) >> shift) & 2047u) + 1u];
                for (uint32_t d = 0; d < 2048; ++d) cnt[d + 1] += cnt[d];
                for (size_t j = 0; j < key.size(); ++j) dst[cnt[(((src[j] >> 24) - lo) >> shift) & 2047u]++] = src[j];
                std::swap(src, dst);
            }
            if (src != key.data()) memcpy(key.data(), src, key.size() * sizeof(uint64_t));
        }
        for (size_t j = 0; j < k.n_small; ++j) k.order[j] = (uint32_t)(key[j] & 0xffffffu);
    } else {                                                     // an index does not fit the key's 24 bits
        std::stable_sort(k.order.begin(), k.order.end(), [&](uint32_t a, uint32_t b) { return aln_pair_cost(k.descs[a]) > aln_pair_cost(k.descs[b]); });
        for (uint32_t i : k.order) cost_sum += (double)aln_pair_cost(k.descs[i]);
    }
    k.max_cells = 0;
    for (uint32_t i : k.order) if (k.descs[i].status == ALN_OK) k.max_cells = std::max(k.max_cells, (uint64_t)k.descs[i].N * k.descs[i].M);
    return cost_sum;
}

// ---------------------------------------------------------------- grid, walk, sharing
// Step 5: persistent waves, 4 per workgroup; and the overlapped traceback: the walk kernel runs beside the fill.  The fast fill
// kernel is built for 160 VGPRs, three workgroups per CU, so that every SIMD keeps 32 registers free: exactly one wave of the walk
// kernel (32 VGPRs, no LDS).  ALN_TB_OVERLAP: unset = one walk wave per SIMD beside a full fill grid; 0 = off; n > 0 = the earlier
// scheme (the fill grid stops n workgroups short of residency and the walk waves crowd onto those CUs, 20 per slot).
inline void aln_plan_grid(uint32_t cus, const AlnPlanCall &c, const AlnPlanKnobs &kn, bool allow_overlap, Chunk &k)
{
    const uint32_t wg_needed = (uint32_t)((k.n_small + 3) / 4);
    k.grid = std::max(1u, std::min(wg_needed, cus * 4u));
    const uint32_t resident = cus * 3u;
    const uint32_t reserve = kn.tb_overlap.set ? (uint32_t)(int)kn.tb_overlap.v : 0u;
    const bool off = kn.tb_overlap.set && reserve == 0;
    // (only where the fill is long enough to hide anything behind: the walk waves, their 30 us head start and the
    // write-through stores cost a batch of 10 000 read pairs -- 0.3 ms of fill -- 40 % of its time)
    k.overlap = allow_overlap && !off && c.fast && c.is_int && c.want_tb && c.store_dirs && reserve < resident &&
                k.n_small >= 4096 && wg_needed >= resident && (k.cells >= 2000000000ull || kn.tb_overlap_any);
    k.counter_bytes = 256;
    if (k.overlap) {
        k.grid = resident - reserve;
        k.tb_waves = reserve ? reserve * 20u : cus * 4u;
        k.counter_bytes = 256 + 4ull * k.n_small;
    }
}

// Which build of the fast batch kernel a chunk that could share strips runs: with the cooperative machinery (COOP = true) or
// without it (the lean build).
//
// With more than two pairs per resident wave nobody opens a first pass (FillArgs::coop_tail); what can still be shared are the
// re-fills opened while fewer than two pairs per kernel wave are left in the queue (fast_work: taken + 2 x waves >= pairs) --
// re-fills of the pairs whose first pass ends then.  In an LPT queue (longest first) those are
//   * the pairs of the queue's tail, its last 2 x waves positions: the first of them is the longest, and
//   * pairs taken early whose first pass lasts into the tail: only a pair that costs a good part of a wave's share can.
// So the lean build is chosen when there are many pairs per resident wave, the tail's longest pair is a small fraction of a
// wave's share (a re-fill of it, alone on one wave, delays little), and the queue's longest pair is at most a quarter of a
// wave's share (its first pass and a re-fill are through before the tail begins, so no build could have shared that re-fill).
// Sharing there shortens next to nothing, while the machinery is paid for in every step of every pair (C5, 100 000 pairs:
// 14.26 against 14.08 VALU instructions per cell, 46.4 against 43.5 GB per launch, fill 45.4 against 43.9 ms).
//
// Costs are in aln_pair_cost units (the time one wave needs for the pair); cost_at(j) = cost of queue position j, the
// queue in LPT order.  grid: the kernel's workgroups of four waves; cus: the device's CUs (three workgroups each are resident).
// setting: ALN_COOP_LEAN (< 0 unset, 0 never lean, > 0 always lean).
static constexpr uint64_t ALN_LEAN_MIN_PAIRS_PER_WAVE = 16;   // at least this many pairs per resident wave
static constexpr double ALN_LEAN_TAIL_FRACTION = 1.0 / 64.0;  // the tail's longest pair: at most this share of a wave's work
static constexpr double ALN_LEAN_MAX_FRACTION = 1.0 / 4.0;    // the queue's longest pair: at most this share

struct AlnLeanPlan {
    uint64_t waves, resident, tail;    // kernel waves, resident waves, queue position of the tail's first (longest) pair
    double share;                      // a resident wave's share of the batch (aln_pair_cost units)
    bool lean;
};

template <class CostAt>
inline AlnLeanPlan aln_coop_lean_plan(uint64_t n_pairs, uint32_t grid, uint32_t cus, double total_cost, CostAt cost_at, int setting)
{
    AlnLeanPlan p;
    p.waves = (uint64_t)grid * 4u;
    p.resident = (uint64_t)cus * 3u * 4u;
    p.tail = n_pairs > 2 * p.waves ? n_pairs - 2 * p.waves : 0;
    const uint64_t w = p.waves < p.resident ? p.waves : p.resident;
    p.share = w ? total_cost / (double)w : 0.0;
    if (setting >= 0) p.lean = setting > 0;
    else if (w == 0 || n_pairs == 0 || n_pairs < ALN_LEAN_MIN_PAIRS_PER_WAVE * w) p.lean = false;
    else p.lean = (double)cost_at((size_t)p.tail) <= ALN_LEAN_TAIL_FRACTION * p.share &&
                  (double)cost_at((size_t)0) <= ALN_LEAN_MAX_FRACTION * p.share;
    return p;
}
// what aln_plan_share found, for the host's ALN_TRACE_PLAN line
struct AlnShareTrace {
    bool could_share = false;          // the chunk could share, so lp holds the figures that chose its build
    AlnLeanPlan lp{};
};

// bytes of the cooperative control block of a grid: control words, one claim word per fill wave (padded to a multiple of 64), one
// record per fill wave
inline uint64_t aln_coop_bytes(uint64_t grid)
{
    return 4ull * (ALN_COOP_CTL_WORDS + ((grid * 4 + 63) & ~63ull)) + grid * 4 * ALN_COOP_REC_BYTES;
}

// Step 6.  Cooperative passes: waves without a pair of their own take strips of other waves' pairs, so a batch with fewer pairs
// than resident waves still gets as many waves as it has strips
// (nothing to share in a batch whose pairs all have one strip -- read pairs, PWM windows, the p-value batch: the kernel then runs
// exactly as without the machinery)
inline void aln_plan_share(uint32_t cus, const AlnPlanCall &c, const AlnPlanKnobs &kn, bool allow_overlap, bool many_chunks, double cost_sum,
                           Chunk &k, AlnShareTrace *trace)
{
    uint64_t strips = 0, multi = 0;
    for (size_t j = 0; j < k.n_small; ++j) {
        const PairDesc &d = k.descs[k.order[j]];
        // (a pair has something to share when its first pass has several strips, or when it may be re-filled -- core local with
        // del != ext -- and is large enough for that re-fill to matter: a 330 x 300 window is through in 40 us either way)
        if (d.status == ALN_OK) {
            strips += aln_num_strips(d.M);
            multi += (d.M > ALN_STRIP_ROWS || (c.hazard && d.M > 64u && (uint64_t)d.N * d.M >= (1u << 18))) ? 1u : 0u;
        }
    }
    // (one of many chunks of a pipelined call: its tail hides behind the chunks after it, and sharing re-fills only cost -- measured on
    // C5 through aln_align_batch, eight chunks: 51.2 ms without, 52.0 with; three chunks of the 12 500-pair shard: 10.3 without, 9.3 with)
    k.coop = aln_coop_on(c, kn) && k.n_small != 0 && multi != 0 && !many_chunks;
    // Many pairs per wave and a queue whose tail is short pairs: next to nothing would be shared -- the lean build.
    // (C5, 100 000 pairs: 33 per resident wave, the tail's longest re-fill 0.7 % of a wave's share)
    // (k.grid as the kernel will run it: the overlapped traceback has already cut it to the resident workgroups)
    if (k.coop) {
        const AlnLeanPlan lp = aln_coop_lean_plan(k.n_small, k.grid, cus, cost_sum, [&](size_t j) { return aln_pair_cost(k.descs[k.order[j]]); },
                                                  kn.coop_lean);
        if (trace) { trace->could_share = true; trace->lp = lp; }
        if (lp.lean) {
            k.coop = false;
            k.coop_lean = true;
        }
    }
    if (k.coop) {
        const uint32_t resident = cus * 3u;
        // (allow_overlap == false: a chunk of a pipelined call -- the chunks before and after it share the chip with this one, so its
        // grid stays at one wave per pair, nobody lingers, and only re-fills are shared)
        const bool alone = allow_overlap;
        if (!k.overlap && alone) k.grid = std::max(k.grid, (uint32_t)std::min<uint64_t>(resident, (strips + 3) / 4));
        // First passes give strips away only in batches of fewer than two pairs per resident wave -- there the pairs that are still
        // running when the queue is dry are large, and idle waves are what fills the chip.  In a larger batch the last pairs are the
        // shortest ones (measured on the 12 500-pair shard of C5: opening the first passes of its last 6000 pairs cost 0.15 ms of 6.8
        // and shortened nothing); re-fills are always shared.  ALN_COOP_TAIL overrides (pairs from the end whose first pass is opened).
        uint64_t tail = (alone && k.n_small < 2ull * resident * 4u) ? k.n_small : 0;
        if (kn.coop_tail.set) tail = (uint64_t)kn.coop_tail.v;
        k.coop_tail = (uint32_t)(k.n_small > tail ? k.n_small - tail : 0);
        // waves that find the queue dry stay around for strips only when they are what fills the chip: a batch with fewer pairs than
        // resident waves (measured on the 12 500-pair shard: staying costs the waves that still work 0.2 ms of 7)
        k.coop_linger = alone && k.n_small < (uint64_t)resident * 4u;
        // Chains of strips (every first pass open, two or more strips per pair on average, no more pairs than resident waves) run
        // with TWO waves per SIMD: a chain is as fast as its slowest strip, and the third wave of a SIMD is the one the arbiter
        // leaves out (256 / 512 / 1024 pairs of 4200 x 4200, score only: 4.97 / 8.99 / 11.8 -> 4.47 / 7.82 / 10.6 ms; 3072 pairs
        // 23.9 -> 22.8; 5000 pairs -- a wave per pair -- 32.8 -> 36.1: not there).  ALN_CHAIN_WGS=0: off.
        if (alone && !k.overlap && tail >= k.n_small && k.n_small <= (uint64_t)resident * 4u && strips >= 2 * k.n_small &&
            !(kn.chain_wgs.set && kn.chain_wgs.v == 0))
            k.grid = std::min(k.grid, cus * 2u);
    }
    if (kn.fill_wgs.set) k.grid = std::max(1u, std::min(k.grid, (uint32_t)(int)kn.fill_wgs.v));   // experiments: fewer resident fill waves
    if (k.coop) k.coop_bytes = aln_coop_bytes(k.grid);
}

// ---------------------------------------------------------------- scratch, LDS, two pairs per wave
// boundary rows in each wave's scratch: fast kernels: a strip never writes the row it reads -- two rows; hazard pairs: strip 0's
// bottom row keeps one more to itself (the localized repair of the row-1 hazard, do_pair_fast, compares against it)
inline uint32_t aln_cascade_rows(const AlnPlanCall &c) { return (c.fast && c.hazard) ? ALN_CASCADE_ROWS : (c.fast ? 2u : 1u); }
// bytes of one wave's scratch for pairs of at most max_len rows or columns: boundary rows, advice, bottom-row record,
// checkpoints, row 1
inline uint64_t aln_scratch_stride(const AlnPlanCall &c, uint64_t max_len, uint64_t *zrow = nullptr)
{
    const uint64_t sc_size = (c.is_int && !c.fast) ? 4 : 8;          // fast kernels: 8-byte granules {T value, tag}
    const uint64_t brow_bytes = ((max_len + 66) * sc_size + 63) & ~63ull;
    const uint64_t adv_bytes = (max_len + 66 + 63) & ~63ull;
    // fast path, hazard pairs: strip 0 checkpoints its lane state (18 ints x 64 lanes per checkpoint)
    const uint64_t ck_bytes = c.fast ? (uint64_t)ALN_CK_SLOTS * 18 * 64 * 4 : 0;
    // bottom-row record: one byte per column (generic kernels) or one direction dword per block of the last strip (fast
    // path: at most (max_len + 63) / 2 + 4 blocks)
    const uint64_t zrow_bytes = std::max<uint64_t>(adv_bytes, ((c.fast ? 8ull : 4ull) * ((max_len + 63) / 2 + 8) + 63) & ~63ull);
    if (zrow) *zrow = zrow_bytes;
    // generic kernels: row 1 as the pass computed it (values + direction tags), for adopt_advice_checked
    const uint64_t row1_bytes = c.fast ? 0 : brow_bytes + adv_bytes;
    return (uint64_t)aln_cascade_rows(c) * brow_bytes + adv_bytes + zrow_bytes + ck_bytes + row1_bytes;
}

// Step 7: a wave's scratch and the batch kernel's LDS
inline void aln_plan_scratch_lds(const AlnPlanCall &c, Chunk &k)
{
    uint64_t zrow_bytes = 0;
    k.cascade_rows = aln_cascade_rows(c);
    k.scratch_stride = aln_scratch_stride(c, k.max_len, &zrow_bytes);
    k.zrow_bytes = (uint32_t)zrow_bytes;
    k.lds_bytes = c.pair_matrices ? aln_pairset_lds_bytes(c.rows, c.cols) : (uint32_t)(((uint64_t)c.rows * c.cols * (c.is_int ? 4 : 8) + 15) & ~15ull);
    k.prof_stride = 0;
    if (c.fast && !c.pwm) { k.prof_stride = c.cols * 64u * ALN_FULL_R; k.lds_bytes = aln_fast_lds_bytes(c.rows, c.cols, k.prof_stride, ALN_FEED_BYTES); }
}

// Step 8.  Two short pairs per wave (core global, read pairs: aln_fill_duo_kernel): every pair of the queue at most 256 rows and
// 1024 columns, more pairs than resident waves (with fewer, a wave per pair is through sooner), nothing shared, no walk waves
// beside the fill, and the staged queries fit beside the profiles with three workgroups per CU.  ALN_NO_DUO=1: off.
inline void aln_plan_duo(uint32_t cus, const AlnPlanCall &c, const AlnPlanKnobs &kn, Chunk &k)
{
    k.duo_qo = 0;
    if (!(c.fast && !c.pwm && c.semantics == ALN_CORE_GLOBAL && !k.coop && !k.coop_lean && !k.overlap && !kn.no_duo && k.n_small > (uint64_t)cus * 12u))
        return;
    uint32_t max_rows = 0, max_cols = 0;
    for (size_t j = 0; j < k.n_small; ++j) { const PairDesc &d = k.descs[k.order[j]]; max_rows = std::max(max_rows, d.M); max_cols = std::max(max_cols, d.N); }
    const uint32_t qo = (max_cols + 136u + 7u) & ~7u;
    // (a wave's profile: R = ceil(rows / 32) bytes per lane and code, rounded up to 1 / 2 / 4 / 8 -- 20-letter alphabets fit with
    // up to 128 rows)
    const uint32_t rmax = (max_rows + 31u) / 32u, rp = rmax > 4u ? 8u : rmax > 2u ? 4u : std::max(rmax, 1u);
    const uint32_t prof = c.cols * 64u * rp;
    const uint32_t lds = (uint32_t)(((uint64_t)c.rows * c.cols * 4 + 15) & ~15ull) + 4u * (prof + 4u * qo);
    if (max_rows <= 256u && max_cols <= 1024u && lds <= 52u * 1024u) {
        k.duo_qo = qo;
        k.prof_stride = prof;
        k.lds_bytes = lds;
        const uint32_t items = (uint32_t)((k.n_small + 1) / 2);
        k.grid = std::max(1u, std::min((items + 3u) / 4u, cus * 3u));
    }
}

// ---------------------------------------------------------------- the plan of one chunk
// Pairs [first, first + n) of the call's tables, on a device of `cus` CUs.  allow_overlap: the chunk has the device to itself (a
// single-chunk call, a staged batch).  many_chunks: one of more than four chunks of a pipelined call.  k: a fresh or reset() Chunk.
inline void aln_plan_chunk(uint32_t cus, const AlnPlanCall &c, const AlnPlanKnobs &kn, const uint64_t *q_off, const uint64_t *q_len,
                           const uint64_t *t_off, const uint64_t *t_len, size_t first, size_t n, bool allow_overlap, bool many_chunks, Chunk &k,
                           AlnShareTrace *trace = nullptr)
{
    aln_plan_descs(c, q_off, q_len, t_off, t_len, first, n, k);
    aln_plan_routes(c, kn, aln_big_to_single(cus, c, kn, k), k);
    const double cost_sum = aln_plan_order(k);
    aln_plan_grid(cus, c, kn, allow_overlap, k);
    aln_plan_share(cus, c, kn, allow_overlap, many_chunks, cost_sum, k, trace);
    aln_plan_scratch_lds(c, k);
    aln_plan_duo(cus, c, kn, k);
}

// ---------------------------------------------------------------- bounds over a range of pairs
// Upper bounds over the chunks of a pipelined call: a slot is sized for the largest chunk the first time it is touched, so no
// buffer grows (hipFree + hipMalloc stall every stream) in the middle of the pipeline.  aln_plan_bounds: what any plan of pairs
// [first, first + n) on a device of at most `cus` CUs can ask for; raise(): the maximum over ranges.
struct AlnPlanBounds {
    uint64_t seq_span = 0, n = 0, dir_bytes = 0, tb_bytes = 0, tag_bytes = 0, scratch = 0, coop = 0;
    void raise(const AlnPlanBounds &o)
    {
        seq_span = std::max(seq_span, o.seq_span); n = std::max(n, o.n); dir_bytes = std::max(dir_bytes, o.dir_bytes);
        tb_bytes = std::max(tb_bytes, o.tb_bytes); tag_bytes = std::max(tag_bytes, o.tag_bytes); scratch = std::max(scratch, o.scratch);
        coop = std::max(coop, o.coop);
    }
};
inline AlnPlanBounds aln_plan_bounds(uint32_t cus, const AlnPlanCall &c, const uint64_t *q_off, const uint64_t *q_len, const uint64_t *t_off,
                                     const uint64_t *t_len, size_t first, size_t n)
{
    AlnPlanBounds b;
    AlnSeqSpan span;
    uint64_t mlen = 1;
    for (size_t i = first; i < first + n; ++i) {
        const uint64_t N = c.pwm ? c.cols : q_len[i], M = t_len[i], cap = N + M + 2;
        span.add_pair(c.pwm, q_off[i], q_len[i], t_off[i], t_len[i]);
        if (c.store_dirs) { b.tb_bytes += aln_tb_bytes(c.pwm, cap); b.tag_bytes += aln_tag_bytes(cap); }
        if (N && M && c.store_dirs) b.dir_bytes += aln_dir_bytes((uint32_t)N, (uint32_t)M);
        if (N && M) mlen = std::max(mlen, std::max(N, M));
    }
    b.seq_span = span.bytes();
    b.n = n;
    // the largest grid is four workgroups of four waves per CU; the claim words' padding at its most
    const uint64_t waves = (uint64_t)cus * 16;
    if (c.fast) b.coop = 4ull * (ALN_COOP_CTL_WORDS + waves + 64) + waves * ALN_COOP_REC_BYTES;
    b.scratch = waves * aln_scratch_stride(c, mlen);
    return b;
}

// ---------------------------------------------------------------- chunking of a batch call
// Chunks are ranges of the caller's pair order, between 5e9 and 1.6e10 cells each (1.4-4.6 GB of packed directions, 2-6 ms
// of fill): small enough that the first upload and the last traceback + download -- the only stages nothing overlaps -- are a
// few per cent of a large call, large enough that a chunk fills the chip and that its largest pairs (a 2000 x 2000 pair takes
// ~3 ms on its wave whatever else runs) do not outlast it by much.  ALN_CHUNK_CELLS overrides (aln_chunk_cells_override).
// Measured (profiles/r02_e2e_chunking.txt): C5 100 000 pairs (47.3 ms resident): 30 chunks 60 ms, 16 chunks 54 ms, 8 chunks 52 ms;
// 25 000 pairs: 6 chunks 18.2 ms, 2-4 chunks 16.6-17.1, one chunk 21.1; 12 500 pairs: 7 chunks 15.6 ms, 3 chunks 9.7, one 10.7.
// total: the cells of all n pairs; ndev: the devices that share the chunks; waves: the resident waves of one device.
inline double aln_chunk_target(bool fast, double total, uint64_t n, size_t ndev, double waves)
{
    // (several devices: the same bounds per device -- each takes about three chunks or more from the common queue)
    double target = std::min(1.6e10, std::max(5.0e9, total / (4.0 * (double)ndev)));
    // The generic (f64 / off-fast-path) kernels take ~3 x as long per cell and have no cooperative passes: a chunk ends with its
    // largest pairs alone on their waves for 10-30 ms, so what counts is pairs per wave, not overlap of the copies (r03, 20 000
    // real-valued C5 pairs: four chunks 44.6 ms, one 40.7, resident 29.9).
    if (!fast) target *= 3.0;
    // Large pairs: what a chunk needs is pairs, not cells -- two or more per resident wave, or the whole batch, so that either every
    // wave has pairs of its own or the chunk is alone on the chip and its waves share the strips of a pair (cooperative passes are
    // for a kernel that has the chip to itself).  r03, 1024 pairs of 4200 x 4200, score only: four chunks of 284 pairs 31 ms (one
    // wave per pair, 9 strips one after the other), one chunk 11.2 ms; 2000 pairs 31 -> 17.3 ms; 512 pairs 15.7 -> 8.9 ms.  Large
    // pairs carry few bytes per cell, so the copies that chunking would overlap are small; the cap keeps a chunk's packed directions
    // at 16 GB (four slots).
    // (pairs of C5's size -- 1.2e6 cells on average -- keep the bounds above: they were measured on them)
    if (n && total / (double)n >= 3.0e6) target = std::max(target, std::min(6.4e10, 2.0 * waves * (total / (double)n)));
    return target;
}
// a shuffle call's chunks (copies of the call's targets, cut by shuffle_chunks): the upper cell bound of aln_chunk_target, flat
inline double aln_shuffle_chunk_target(bool fast) { return fast ? 1.6e10 : 4.8e10; }
// ALN_CHUNK_CELLS: a target set by hand; *forced then also lifts the one-chunk floors (tests cut small batches into chunks)
inline double aln_chunk_cells_override(const AlnPlanKnobs &kn, double target, bool *forced = nullptr)
{
    if (forced) *forced = kn.chunk_cells_set;
    return kn.chunk_cells_set ? std::max(1.0, kn.chunk_cells) : target;
}

inline void aln_make_chunks(const AlnPlanCall &c, const AlnPlanKnobs &kn, const uint64_t *q_len, const uint64_t *t_len, size_t n, size_t ndev,
                            std::vector<std::pair<size_t, size_t>> &out, double waves = 3072.0)
{
    out.clear();
    auto pair_cells = [&](size_t i) { return (double)(c.pwm ? c.cols : q_len[i]) * (double)t_len[i]; };
    double total = 0;
    for (size_t i = 0; i < n; ++i) total += pair_cells(i);
    bool forced = false;
    const double target = aln_chunk_cells_override(kn, aln_chunk_target(c.fast, total, n, ndev, waves), &forced);
    // (one chunk up to 2e10 cells: a one-chunk call uploads its residues while it plans and its kernel has the chip to itself -- 12 500
    // C5 pairs, 1.5e10 cells: 8.7 ms against 9.1-9.4 in three chunks; 25 000 pairs, 3e10: 17 against 15.5 in four)
    // -- unless the strings it brings back are many: nothing overlaps that copy in a one-chunk call (100 000 PWM windows with both
    // strings, 316 MB: 15.3 ms in one chunk, 13.2 in two)
    double out_bytes = 0;
    if (c.want_tb) for (size_t i = 0; i < n; ++i) out_bytes += (c.pwm ? 5.0 : 2.0) * ((double)(c.pwm ? c.cols : q_len[i]) + (double)t_len[i] + 2.0);
    if (!forced && total <= std::max(1.5 * target, 2.0e10) && ndev == 1 && out_bytes <= 64.0e6) { out.emplace_back(0, n); return; }
    if (total <= 1.5 * target) { out.emplace_back(0, n); return; }
    size_t first = 0;
    double acc = 0;
    for (size_t i = 0; i < n; ++i) {
        acc += pair_cells(i);
        if (acc >= target || i + 1 - first >= (1u << 22)) { out.emplace_back(first, i + 1 - first); first = i + 1; acc = 0; }
    }
    if (first < n) {
        // a short tail joins the chunk before it
        if (!out.empty() && acc < 0.25 * target) out.back().second += n - first;
        else out.emplace_back(first, n - first);
    }
}
