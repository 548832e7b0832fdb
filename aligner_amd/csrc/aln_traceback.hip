// aln_traceback.hip -- gfx950 kernels that read the packed direction store the fill kernels (aln_kernels.hip) wrote: the batch walks
// (one lane per pair, one wave per pair, the walk beside the fill), the parallel traceback of one large pair (exit maps, chain,
// segments), the expansion of a tag string into the two aligned code strings, the direction unpack -- and the exact rescaling of
// the summaries of a dyadic scheme.  Nothing here uses the fill templates: the layout is aln_device.h's and aln_layout_rules.h's.
// One translation unit, one code object (aln_warm_tb).
#include <hip/hip_runtime.h>

#include "aln_device.h"
#include "aln_launch.h"

// ---------------------------------------------------------------- traceback
// Direction of cell (y, x) from the packed store (borders are implicit: simple/mod.rs:55-67).
__device__ __forceinline__ int dir_at(const uint8_t *dirs, const PairDesc &d, bool global, uint32_t y, uint32_t x)
{
    if (y == 0 || x == 0) {
        if (!global || (y == 0 && x == 0)) return D_BEG;
        return y == 0 ? D_LEFT : D_TOP;
    }
    const uint8_t *base = dirs + d.dir_off;
    if (d.layout == ALN_LAYOUT_ROWMAJOR) {
        const uint32_t rowbytes = (d.N + 4) / 4;
        return (base[(size_t)y * rowbytes + (x >> 2)] >> (2 * (x & 3u))) & 3;
    }
    uint32_t strip, i;
    int R;
    uint64_t strip_bytes;
    if ((d.layout & 0xffu) == ALN_LAYOUT_UNIFORM || (d.layout & 0xffu) == ALN_LAYOUT_UBATCH) {
        R = (int)((d.layout >> 8) & 0xffu);
        strip = (y - 1) / (64u * R);
        i = (y - 1) - strip * 64u * R;
        strip_bytes = aln_uniform_strip_bytes(d.N, (uint32_t)R);
    } else {
        strip = (y - 1) / ALN_STRIP_ROWS;
        const uint32_t ns = aln_num_strips(d.M);
        R = (strip + 1 == ns) ? aln_pick_r(d.M - strip * ALN_STRIP_ROWS) : ALN_FULL_R;
        i = (y - 1) - strip * ALN_STRIP_ROWS;
        strip_bytes = aln_strip_bytes(d.N);
    }
    const uint32_t lane = i / R, r = i % R;
    const uint32_t k = (x - 1) + lane;
    const uint32_t spb = aln_spb((uint32_t)R);
    const uint32_t *wbase = reinterpret_cast<const uint32_t *>(base + strip * strip_bytes);
    const uint32_t word = wbase[aln_dir_word_index(k, lane, spb)];
    return aln_tag_to_dir((int)((word >> aln_dir_bitpos(k, r, lane, d.N, R)) & 3u));
}

// Per-strip constants of the packed direction store, re-derived only when the walk leaves the strip.
struct StripView {
    const uint32_t *wbase;
    uint32_t y0;        // rows of the strip are y0+1 .. y0+rows
    uint32_t R;         // rows per lane (1..8; the uniform layout of the single-pair route: a power of two)
    uint32_t lgS;       // log2(steps per direction word)
};
__device__ __forceinline__ StripView strip_view(const uint8_t *dirs, const PairDesc &d, uint32_t y)
{
    StripView v;
    const uint8_t *base = dirs + d.dir_off;
    if ((d.layout & 0xffu) == ALN_LAYOUT_UNIFORM || (d.layout & 0xffu) == ALN_LAYOUT_UBATCH) {
        v.R = (d.layout >> 8) & 0xffu;
        const uint32_t strip = (y - 1) / (64u * v.R);
        v.y0 = strip * 64u * v.R;
        v.wbase = reinterpret_cast<const uint32_t *>(base + strip * aln_uniform_strip_bytes(d.N, v.R));
    } else {
        const uint32_t strip = (y - 1) / ALN_STRIP_ROWS;
        const uint32_t ns = aln_num_strips(d.M);
        v.R = (strip + 1 == ns) ? (uint32_t)aln_pick_r(d.M - strip * ALN_STRIP_ROWS) : (uint32_t)ALN_FULL_R;
        v.y0 = strip * ALN_STRIP_ROWS;
        v.wbase = reinterpret_cast<const uint32_t *>(base + strip * aln_strip_bytes(d.N));
    }
    v.lgS = 31u - (uint32_t)__builtin_clz(aln_spb(v.R));
    return v;
}

// One thread per pair: the reference's pointer chase (simple/mod.rs:99-130, :213-245; legacy :146-176, :232-261),
// including the duplicated seed pair.  Pass 1 is the dependent chain -- one direction word per step, shifts only, the
// 2-bit tags go to a scratch byte string; pass 2 turns the tags into the two aligned code strings, written in final
// (forward) order, with loads whose addresses do not depend on loaded data.
__device__ __forceinline__ void tb_walk_pair(const TraceArgs &a, uint32_t pair)
{
    const PairDesc &d = a.descs[pair];
    aln_pair_result &res = a.results[pair];
    if (res.status != ALN_OK) return;
    if ((d.layout & 0xffu) == ALN_LAYOUT_UNIFORM) return;      // large pairs: aln_tb_single_* kernels
    uint8_t *__restrict__ ops = a.tags + d.tag_off;
    const bool global = (a.semantics == ALN_CORE_GLOBAL || a.semantics == ALN_LEGACY_GLOBAL);
    const bool legacy = (a.semantics == ALN_LEGACY_GLOBAL || a.semantics == ALN_LEGACY_LOCAL);
    const uint32_t ey = res.end_y, ex = res.end_x, N = d.N;
    uint32_t cy = ey, cx = ex;
    if (legacy) { cy -= 1; cx -= 1; }   // legacy starts at the diagonal predecessor (aligner_core.rs:146-147, :232-233)
    uint32_t len = 0;                   // steps taken (the seed pair is added in pass 2)
    if (d.layout == ALN_LAYOUT_ROWMAJOR) {
        for (;;) {
            const int dd = dir_at(a.dirs, d, global, cy, cx);
            if (dd == D_BEG) break;
            ops[len++] = (uint8_t)aln_dir_to_tag(dd);
            cy -= (dd != D_LEFT); cx -= (dd != D_TOP);
        }
    } else {
        // The walk is one dependent chain: ~a quarter of a load per step (a lane's quad -- 4 blocks, 16 B -- covers 64/R
        // consecutive steps of R rows and stays in registers until the path leaves it) and the instructions between two
        // loads, which a lone wave issues at one per ~4.6 cycles.  So the step is kept short: the state is (row within the
        // strip, column - 1), both signed -- one sign test catches "left the strip upwards" and both borders.
        if (cy != 0 && cx != 0) {
            StripView sv = strip_view(a.dirs, d, cy);
            int iy = (int)(cy - 1 - sv.y0), cxm = (int)cx - 1;
            // rows per lane R is any of 1..8: lane = iy / R by multiplication (iy < 512), everything about the steps by shifts
            uint32_t R = sv.R, rinv = (65535u + R) / R, lgS = sv.lgS, qsh = lgS + 2u, bmask = (1u << lgS) - 1u;
            const uint4 *wq = reinterpret_cast<const uint4 *>(sv.wbase);
            const uint32_t Nm1 = N - 1u;
            uint32_t qcur = 0xffffffffu;
            uint4 quad = make_uint4(0, 0, 0, 0);
            uint8_t *p = ops;
            for (;;) {
                if ((iy | cxm) < 0) {                       // above the strip, or a border
                    cy = (uint32_t)(iy + 1) + sv.y0; cx = (uint32_t)(cxm + 1);
                    if (cy == 0 || cx == 0) break;
                    sv = strip_view(a.dirs, d, cy);
                    iy = (int)(cy - 1 - sv.y0);
                    R = sv.R; rinv = (65535u + R) / R; lgS = sv.lgS; qsh = lgS + 2u; bmask = (1u << lgS) - 1u;
                    wq = reinterpret_cast<const uint4 *>(sv.wbase);
                    qcur = 0xffffffffu;
                }
                const uint32_t lane = ((uint32_t)iy * rinv) >> 16, r = (uint32_t)iy - lane * R;
                const uint32_t k = (uint32_t)cxm + lane;
                const uint32_t qi = ((k >> qsh) << 6) + lane;
                if (qi != qcur) { quad = wq[qi]; qcur = qi; }
                // the cell's tag sits at bit 32 - 2 R (m + 1) + 2 r of its word, m = steps of this lane left in the block
                // after step k (aln_dir_bitpos); the word is number (k >> lgS) & 3 of the quad
                const uint32_t lend = lane + Nm1;
                const uint32_t m = min(k | bmask, lend) - k;
                const uint32_t j = (k >> lgS) & 3u;
                const uint64_t half = (j & 2u) ? (((uint64_t)quad.w << 32) | quad.z) : (((uint64_t)quad.y << 32) | quad.x);
                const uint32_t tag = (uint32_t)(half >> (32u * (j & 1u) + 32u - 2u * R * (m + 1u) + 2u * r)) & 3u;
                if (tag == 3u) {                            // Beginning
                    cy = (uint32_t)(iy + 1) + sv.y0; cx = (uint32_t)(cxm + 1);
                    break;
                }
                *p++ = (uint8_t)tag;
                iy -= (tag != 1u); cxm -= (tag != 2u);      // 0 Diagonal, 1 Left, 2 Top
            }
            len = (uint32_t)(p - ops);
        }
        if (global) {                                   // borders: D[0][x] = Left, D[y][0] = Top (simple/mod.rs:59-67)
            while (cx != 0 && cy == 0) { ops[len++] = 1; cx--; }
            while (cy != 0 && cx == 0) { ops[len++] = 2; cy--; }
        }
    }
    res.start_y = cy; res.start_x = cx;
    res.aln_len = len + (a.pwm ? 0u : 1u);              // + the duplicated seed pair (none for the PWM aligner)
}
extern "C" __global__ __launch_bounds__(64) void aln_traceback_kernel(TraceArgs a)
{
    const uint32_t pair = blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= a.n_pairs) return;
    if (a.walked && a.walked[pair] == a.epoch) return;  // the overlap kernel has been here
    // latency-bound and light on issue slots: ahead of the fill waves (of the next chunk) it shares a SIMD with
    __builtin_amdgcn_s_setprio(3);
    tb_walk_pair(a, pair);
}
// ---------------------------------------------------------------- one WAVE per pair: the walk of a batch of few, long pairs
// aln_traceback_kernel's walk waits for memory once per direction quad (a dependent 16-byte load every 4-8 steps, ~2 us when it comes
// from HBM: 3.7 ms for the 8400-step paths of 256 pairs of 4200 x 4200 -- as long as their fill); with one pair per lane that is
// the price of 64 walks in flight, with 256 pairs it is all there is.  Here a wave walks ONE pair and all its lanes fetch ahead:
// wave lane j keeps, for lane j of the strip the path is in, the three quads around the step at which a purely diagonal path from
// the current cell would enter that lane's rows -- one round of loads per strip (the path climbs through the lanes, 64 R rows), a new
// round when gaps have carried it out of the three quads (8+ steps either way).  The state of the walk is wave-uniform: the step
// runs on scalar registers, the quad it needs comes out of the window with v_readlane, the tags leave 64 at a time.
__device__ __forceinline__ uint32_t uni32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
template <class T>
__device__ __forceinline__ const T *uni_ptr(const T *p)
{
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    return reinterpret_cast<const T *>(((uint64_t)uni32((uint32_t)(v >> 32)) << 32) | uni32((uint32_t)v));
}
__device__ __forceinline__ StripView strip_view_uniform(const uint8_t *dirs, const PairDesc &d, uint32_t y)
{
    StripView v = strip_view(dirs, d, y);                    // (loads of the descriptor: the compiler cannot know they are uniform)
    v.wbase = uni_ptr(v.wbase); v.y0 = uni32(v.y0); v.R = uni32(v.R); v.lgS = uni32(v.lgS);
    return v;
}
__device__ __forceinline__ void tb_walk_pair_wave(const TraceArgs &a, const uint32_t pair)
{
    const PairDesc &d = a.descs[pair];
    aln_pair_result &res = a.results[pair];
    const uint32_t lane_id = threadIdx.x & 63u;
    if (__builtin_amdgcn_readfirstlane(res.status) != ALN_OK) return;
    const uint32_t layout = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.layout);
    if ((layout & 0xffu) == ALN_LAYOUT_UNIFORM) return;      // large pairs of the single-pair route: aln_tb_single_* kernels
    if (layout == ALN_LAYOUT_ROWMAJOR) {                     // strict-order fallback: rare, one lane
        if (lane_id == 0) tb_walk_pair(a, pair);
        return;
    }
    uint8_t *__restrict__ ops = a.tags + d.tag_off;
    const bool global = (a.semantics == ALN_CORE_GLOBAL || a.semantics == ALN_LEGACY_GLOBAL);
    const bool legacy = (a.semantics == ALN_LEGACY_GLOBAL || a.semantics == ALN_LEGACY_LOCAL);
    const uint32_t N = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.N);
    uint32_t cy = (uint32_t)__builtin_amdgcn_readfirstlane((int)res.end_y), cx = (uint32_t)__builtin_amdgcn_readfirstlane((int)res.end_x);
    if (legacy) { cy -= 1; cx -= 1; }
    uint32_t len = 0;
    uint32_t tagv = 0;                                       // lane i: the tag of i steps ago
    if (cy != 0 && cx != 0) {
        StripView sv = strip_view_uniform(a.dirs, d, cy);
        int iy = (int)(cy - 1 - sv.y0), cxm = (int)cx - 1;
        uint32_t R = sv.R, rinv = (65535u + R) / R, lgS = sv.lgS, qsh = lgS + 2u, bmask = (1u << lgS) - 1u;
        const uint4 *wq = reinterpret_cast<const uint4 *>(sv.wbase);
        const uint32_t Nm1 = N - 1u;
        uint32_t nq = ((N + 62u) >> qsh) + 1u;              // quad rows of a strip (steps 0 .. N + 62)
        uint4 wa = make_uint4(0, 0, 0, 0), wb = wa, wc = wa; // quad rows qrow + 1, qrow, qrow - 1 of strip lane `lane_id`
        uint32_t qrow = 0;
        bool have = false;                                   // the window belongs to the current strip
        uint32_t cur_lane = 0xffffffffu, cur_q = 0xffffffffu;
        uint32_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;             // the current quad (uniform)
        for (;;) {
            if ((iy | cxm) < 0) {                            // above the strip, or a border
                cy = (uint32_t)(iy + 1) + sv.y0; cx = (uint32_t)(cxm + 1);
                if (cy == 0 || cx == 0) break;
                sv = strip_view_uniform(a.dirs, d, cy);
                iy = (int)(cy - 1 - sv.y0);
                R = sv.R; rinv = (65535u + R) / R; lgS = sv.lgS; qsh = lgS + 2u; bmask = (1u << lgS) - 1u;
                wq = reinterpret_cast<const uint4 *>(sv.wbase);
                nq = ((N + 62u) >> qsh) + 1u;
                have = false; cur_lane = 0xffffffffu;
            }
            const uint32_t lane = ((uint32_t)iy * rinv) >> 16, r = (uint32_t)iy - lane * R;
            const uint32_t k = (uint32_t)cxm + lane;
            const uint32_t qr = k >> qsh;
            if (lane != cur_lane || qr != cur_q) {           // (uniform) another quad: out of the window
                uint32_t dq = (uint32_t)__builtin_amdgcn_readlane((int)qrow, (int)lane) + 1u - qr;      // 0 / 1 / 2: wa / wb / wc
                if (!have || dq > 2u) {
                    // fetch ahead from here: strip lane j <= lane is entered after t = iy - (j R + R - 1) diagonal steps, at step
                    // k_j = (cxm - t) + j; its R rows take the path down to k_j - (R - 1): the middle quad holds k_j - R / 2
                    const int t = iy - (int)(lane_id * R + R - 1u);
                    const int kj = (cxm - (t > 0 ? t : 0)) + (int)lane_id - (int)(R >> 1);
                    qrow = (uint32_t)(kj > 0 ? kj : 0) >> qsh;
                    if (lane_id == lane) qrow = qr;          // (the lane the path is in: exactly the quad of this step)
                    const bool on = lane_id <= lane;
                    wa = wb = wc = make_uint4(0, 0, 0, 0);
                    if (on && qrow + 1u < nq) wa = wq[((size_t)(qrow + 1u) << 6) + lane_id];
                    if (on && qrow < nq) wb = wq[((size_t)qrow << 6) + lane_id];
                    if (on && qrow >= 1u) wc = wq[((size_t)(qrow - 1u) << 6) + lane_id];
                    have = true;
                    dq = 1u;
                }
                const int li = (int)lane;
                if (dq == 0u) { q0 = __builtin_amdgcn_readlane((int)wa.x, li); q1 = __builtin_amdgcn_readlane((int)wa.y, li); q2 = __builtin_amdgcn_readlane((int)wa.z, li); q3 = __builtin_amdgcn_readlane((int)wa.w, li); }
                else if (dq == 1u) { q0 = __builtin_amdgcn_readlane((int)wb.x, li); q1 = __builtin_amdgcn_readlane((int)wb.y, li); q2 = __builtin_amdgcn_readlane((int)wb.z, li); q3 = __builtin_amdgcn_readlane((int)wb.w, li); }
                else { q0 = __builtin_amdgcn_readlane((int)wc.x, li); q1 = __builtin_amdgcn_readlane((int)wc.y, li); q2 = __builtin_amdgcn_readlane((int)wc.z, li); q3 = __builtin_amdgcn_readlane((int)wc.w, li); }
                cur_lane = lane; cur_q = qr;
                asm volatile("" : "+s"(cur_lane), "+s"(cur_q));      // (scalars: say so)
            }
            const uint32_t lend = lane + Nm1;
            const uint32_t m = min(k | bmask, lend) - k;
            const uint32_t j = (k >> lgS) & 3u;
            const uint64_t half = (j & 2u) ? (((uint64_t)q3 << 32) | q2) : (((uint64_t)q1 << 32) | q0);
            const uint32_t tag = (uint32_t)(half >> (32u * (j & 1u) + 32u - 2u * R * (m + 1u) + 2u * r)) & 3u;
            if (tag == 3u) {                                 // Beginning
                cy = (uint32_t)(iy + 1) + sv.y0; cx = (uint32_t)(cxm + 1);
                break;
            }
            // the tags enter a lane shift register at lane 0 (one DPP move per step; the step counter stays out of vector code, or
            // the compiler moves the whole walk state there): after 64 steps lane i holds the tag of step 63 - i of the group
            tagv = (uint32_t)__builtin_amdgcn_update_dpp((int)tag, (int)tagv, 0x138, 0xf, 0xf, false);
            ++len;
            if ((len & 63u) == 0u) ops[len - 1u - lane_id] = (uint8_t)tagv;
            iy -= (tag != 1u); cxm -= (tag != 2u);           // 0 Diagonal, 1 Left, 2 Top
        }
    }
    if (lane_id < (len & 63u)) ops[len - 1u - lane_id] = (uint8_t)tagv;       // the last, partial group: lane i holds tag len - 1 - i
    if (global) {                                            // borders: D[0][x] = Left, D[y][0] = Top (simple/mod.rs:59-67)
        if (cy == 0 && cx != 0) { for (uint32_t i = lane_id; i < cx; i += 64u) ops[len + i] = 1; len += cx; cx = 0; }
        else if (cx == 0 && cy != 0) { for (uint32_t i = lane_id; i < cy; i += 64u) ops[len + i] = 2; len += cy; cy = 0; }
    }
    if (lane_id == 0) {
        res.start_y = cy; res.start_x = cx;
        res.aln_len = len + (a.pwm ? 0u : 1u);               // + the duplicated seed pair (none for the PWM aligner)
    }
}
extern "C" __global__ __launch_bounds__(256) void aln_traceback_wave_kernel(TraceArgs a)
{
    const uint32_t pair = uni32(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (pair >= a.n_pairs) return;
    if (a.walked && uni32(a.walked[pair]) == a.epoch) return;
    tb_walk_pair_wave(a, pair);
}
// The walks are latency-bound and the fill is issue-bound: this kernel runs BESIDE the fill kernel (second stream; the host
// leaves a few workgroup slots free for it) and walks the pairs in the order the fill finishes them: persistent waves, each
// claims the next 64 entries of the fill's completion queue and waits for them to appear.  A wave that waits too long
// gives up -- nothing depends on this kernel: aln_traceback_kernel runs after the fill and walks whatever is left, so a
// runtime that serializes the two kernels (profilers do) only loses the overlap.
extern "C" __global__ __attribute__((amdgpu_flat_work_group_size(64, 64), amdgpu_num_vgpr(16))) void aln_traceback_overlap_kernel(TraceArgs a)
{
    __builtin_amdgcn_s_setprio(3);       // latency-bound and light on issue slots: ahead of the fill waves it shares a SIMD with
    for (;;) {
        uint32_t base = 0;
        if (threadIdx.x == 0) base = __hip_atomic_fetch_add(a.head, 64u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (base >= a.n_order) return;
        // 64 consecutive entries of the completion queue: they fill within microseconds of each other
        const uint32_t my = base + threadIdx.x;
        uint32_t v = 0;
        const uint64_t t0 = wall_clock64();
        for (;;) {
            if (my < a.n_order && v == 0) v = __hip_atomic_load(a.doneq + my, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (__all(my >= a.n_order || v != 0)) break;
            __builtin_amdgcn_s_sleep(127);
            if (wall_clock64() - t0 > a.wait_ticks) return;
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);         // nothing cached here from before the entries appeared
        if (my < a.n_order) {
            tb_walk_pair(a, v - 1u);
            a.walked[v - 1u] = a.epoch;
        }
    }
}
// one wave that sleeps ~30 us: queued in front of the overlap kernel so that the fill kernel's workgroups are placed first
extern "C" __global__ __launch_bounds__(64) void aln_delay_kernel(uint32_t ticks)
{
    const uint64_t t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}

// ---------------------------------------------------------------- parallel traceback of one large pair
// A window of a strip's packed direction words staged in LDS: quads [q_lo, q_lo + q_n) (a quad = 4 blocks x 64 lanes x
// 4 B = 1 KiB, contiguous in memory: aln_dir_word_index).  A walk moves up and left, i.e. towards smaller wave steps, so
// the window ends at the quad of the largest step the block's walks start from; whatever leaves it falls back to global.
struct StripWindow {
    const uint32_t *wbase;
    const uint32_t *lds;
    uint32_t q_lo, q_n;
};
// cooperative copy (16 B per thread, coalesced) of the window that ends at wave step k_hi; call from every thread
__device__ __forceinline__ StripWindow stage_window(const uint32_t *wbase, uint32_t *lds, uint32_t lds_quads, uint32_t k_hi,
                                                    uint32_t lgR)
{
    StripWindow w;
    const uint32_t sh = 4u - lgR;                                  // log2(steps per block)
    const uint32_t q_hi = k_hi >> (sh + 2);
    w.wbase = wbase; w.lds = lds;
    w.q_n = min(lds_quads, q_hi + 1u);
    w.q_lo = q_hi + 1u - w.q_n;
    const uint4 *src = reinterpret_cast<const uint4 *>(wbase) + (size_t)w.q_lo * 64u;
    uint4 *dst = reinterpret_cast<uint4 *>(lds);
    // blocks of 256 threads, at most 48 quads: 12 x 16 B per thread, all loads in flight before the first LDS write
    const uint32_t n = w.q_n * 64u;
    uint4 v[12];
#pragma unroll
    for (uint32_t j = 0; j < 12; ++j) {
        const uint32_t i = threadIdx.x + j * 256u;
        if (i < n) v[j] = src[i];
    }
#pragma unroll
    for (uint32_t j = 0; j < 12; ++j) {
        const uint32_t i = threadIdx.x + j * 256u;
        if (i < n) dst[i] = v[j];
    }
    __syncthreads();
    return w;
}

// Walks from (cy, cx) while the walk stays inside the strip whose rows are y0+1 .. (uniform-R layout), following the
// same rules as aln_traceback_kernel.  Returns true if the walk ended (Beginning / origin), false if it left the strip
// upwards (then cy == y0).  `ops` (optional) receives the tags.  fetch(kb, lane) returns the direction word of block kb
// of that lane.  The interior loop is branch-lean (one exit test, one load, shifts); the borders of the global
// semantics (D[0][x] = Left, D[y][0] = Top: simple/mod.rs:55-67) are whole runs and are handled after it.
// `cap` (exit maps only): a walk that has not left the strip after that many steps is given up (*gave_up): far from the real
// path the tags are long gap runs, and one thread following a 900-column Left run held up its whole block.
template <class Fetch>
__device__ __forceinline__ bool walk_in_strip(Fetch fetch, uint32_t y0, uint32_t lgR, uint32_t N, bool global,
                                              uint32_t &cy, uint32_t &cx, uint32_t &steps, uint8_t *ops,
                                              uint32_t cap = 0xffffffffu, bool *gave_up = nullptr)
{
    const uint32_t R = 1u << lgR, sh = 4u - lgR;
    uint32_t y = cy, x = cx, n = steps;
    const uint32_t n_stop = cap == 0xffffffffu ? cap : steps + cap;
    bool beginning = false;
    bool go = (y > y0 && x != 0);
    while (go) {                                       // single exit, body predicated: the loop is one exec-mask update
        const uint32_t i = y - 1 - y0;
        const uint32_t lane = i >> lgR, r = i & (R - 1u);
        const uint32_t k = x - 1 + lane, kb = k >> sh;
        const uint32_t word = fetch(kb, lane);
        const uint32_t e = min((kb << sh) + (1u << sh) - 1u, lane + N - 1u);
        const uint32_t tag = (word >> (30u - 2u * (((e - k) << lgR) + (R - 1u - r)))) & 3u;
        beginning = (tag == 3u);
        if (ops && !beginning) ops[n] = (uint8_t)tag;
        n += beginning ? 0u : 1u;
        y -= (tag == 0u || tag == 2u) ? 1u : 0u;       // 0 Diagonal, 1 Left, 2 Top (3 moves nothing)
        x -= (tag <= 1u) ? 1u : 0u;
        go = !beginning && y > y0 && x != 0 && n < n_stop;
    }
    if (gave_up) *gave_up = !beginning && y > y0 && x != 0;
    bool ended = beginning;
    if (!beginning) {
        if (!global) ended = (y == 0 || x == 0);                         // local: every border cell is Beginning
        else if (y == 0) {                                               // top border: Left all the way to the origin
            if (ops) for (uint32_t j = 0; j < x; ++j) ops[n + j] = 1;
            n += x; x = 0; ended = true;
        } else if (x == 0) {                                             // left border: Top until the strip is left
            const uint32_t run = y - y0;
            if (ops) for (uint32_t j = 0; j < run; ++j) ops[n + j] = 2;
            n += run; y = y0; ended = false;
        }
    }
    cy = y; cx = x; steps = n;
    return ended;
}
// LDS quads of the traceback kernels' window: 768 wave steps (48 KiB at most)
__host__ __device__ inline uint32_t tb_window_quads(uint32_t R) { const uint32_t q = 12u * R; return q > 48u ? 48u : q; }

// Exit maps are computed only where the path can plausibly enter a strip: a band of TB_BAND columns around the line of
// slope 1 through the traceback's start cell (insertions push the path left of it, deletions right).  The chain kernel
// uses a map entry when the real entry column falls into the band and walks the strip itself when it does not, so the
// band is a speed choice, never a correctness one.  Strips below the start cell need no map at all.
#define TB_BAND 1024u
__device__ __forceinline__ bool tb_band(uint32_t ey, uint32_t ex, uint32_t yb, uint32_t N, uint32_t &c_lo, uint32_t &c_hi)
{
    if (yb > ey) return false;                                   // the path never enters this strip from below
    const uint32_t dy = ey - yb;
    const uint32_t c = ex > dy ? ex - dy : 0u;                   // column of the slope-1 line on the strip's bottom row
    c_lo = c > TB_BAND / 2u ? c - TB_BAND / 2u : 0u;
    c_hi = min(N, c_lo + TB_BAND - 1u);
    return true;
}

// exit map: thread (x, s) enters strip s on its bottom row at column x; the block's 256 walks share one staged window
extern "C" __global__ __launch_bounds__(256) void aln_tb_single_maps_kernel(TraceSingleArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem_words[];
    const PairDesc &d = a.descs[a.pair];
    if (a.results[a.pair].status != ALN_OK || (d.layout & 0xffu) != ALN_LAYOUT_UNIFORM) return;   // serial fallback: aln_traceback_kernel
    const uint32_t s = blockIdx.y;
    const uint32_t lgR = 31u - (uint32_t)__builtin_clz(a.R), rows = 64u << lgR;
    const uint32_t y0 = s * rows;
    const bool global = (a.semantics == ALN_CORE_GLOBAL || a.semantics == ALN_LEGACY_GLOBAL);
    const bool legacy = (a.semantics == ALN_LEGACY_GLOBAL || a.semantics == ALN_LEGACY_LOCAL);
    const uint32_t *wbase = reinterpret_cast<const uint32_t *>(a.dirs + d.dir_off + s * aln_uniform_strip_bytes(d.N, a.R));
    const uint32_t cy0 = min(d.M, y0 + rows);
    uint32_t c_lo, c_hi;
    if (!tb_band(a.results[a.pair].end_y - (legacy ? 1u : 0u), a.results[a.pair].end_x - (legacy ? 1u : 0u), cy0, d.N, c_lo, c_hi)) return;
    if (c_lo + blockIdx.x * blockDim.x > c_hi) return;           // (uniform over the block)
    const uint32_t x = c_lo + blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t x_hi = min(c_hi, c_lo + blockIdx.x * blockDim.x + blockDim.x - 1u);
    const uint32_t k_hi = (x_hi ? x_hi - 1u : 0u) + ((cy0 - 1u - y0) >> lgR);
    const StripWindow w = stage_window(wbase, smem_words, tb_window_quads(a.R), k_hi, lgR);
    if (x > c_hi) return;
    uint32_t cy = cy0, cx = x, steps = 0;
    const uint32_t q_lo = w.q_lo, q_n = w.q_n;
    // LDS through an address-space-3 pointer: a generic pointer would turn the two loads into one flat_load with a select
    const __attribute__((address_space(3))) uint32_t *lds3 = (const __attribute__((address_space(3))) uint32_t *)smem_words;
    auto fetch = [&](uint32_t kb, uint32_t lane) -> uint32_t {
        const uint32_t q = kb >> 2, rel = q - q_lo;
        uint32_t word = lds3[((min(rel, q_n - 1u) * 64u + lane) << 2) + (kb & 3u)];            // ds_read, always in range
        if (__builtin_expect(rel >= q_n, 0)) word = wbase[(((uint64_t)q * 64u + lane) << 2) + (kb & 3u)];   // left the window (rare)
        return word;
    };
    // a path crosses the strip in rows .. rows + (gap columns) steps; beyond twice the rows + 64 the entry is marked unusable
    // (2) and the chain kernel, should the real path ever come this way, walks the strip itself
    bool gave_up = false;
    const bool stopped = walk_in_strip(fetch, y0, lgR, d.N, global, cy, cx, steps, nullptr, 2u * rows + 64u, &gave_up);
    a.map[(size_t)s * (d.N + 1) + x] = make_uint4(cx, cy, steps, gave_up ? 2u : stopped ? 1u : 0u);
}

// one thread: from the end cell through its own strip, then strip by strip through the maps
extern "C" __global__ void aln_tb_single_chain_kernel(TraceSingleArgs a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const PairDesc &d = a.descs[a.pair];
    aln_pair_result &res = a.results[a.pair];
    for (uint32_t s = 0; s < a.ns; ++s) a.seg[s] = make_uint4(0, 0, 0, 0);
    if (res.status != ALN_OK || (d.layout & 0xffu) != ALN_LAYOUT_UNIFORM) return;
    const uint32_t lgR = 31u - (uint32_t)__builtin_clz(a.R), rows = 64u << lgR;
    const bool global = (a.semantics == ALN_CORE_GLOBAL || a.semantics == ALN_LEGACY_GLOBAL);
    const bool legacy = (a.semantics == ALN_LEGACY_GLOBAL || a.semantics == ALN_LEGACY_LOCAL);
    uint32_t cy = res.end_y, cx = res.end_x;
    if (legacy) { cy -= 1; cx -= 1; }
    const uint32_t cy_start = cy, cx_start = cx;             // the cell the band of the exit maps is centred on
    uint32_t off = 0;
    bool stopped = (cy == 0 || cx == 0) && (!global || (cy == 0 && cx == 0));
    if (!stopped && cy == 0) {                       // only the top border is left (global)
        a.seg[0] = make_uint4(cy, cx, 0, 1);
        off = cx; cx = 0; stopped = true;
    }
    if (!stopped) {
        uint32_t s = (cy - 1) >> (6 + lgR);
        // first segment: from the end cell, which need not be on the strip's bottom row
        a.seg[s] = make_uint4(cy, cx, 0, 1);
        const uint32_t *wbase = reinterpret_cast<const uint32_t *>(a.dirs + d.dir_off + s * aln_uniform_strip_bytes(d.N, a.R));
        auto fetch = [&](uint32_t kb, uint32_t lane) -> uint32_t { return wbase[(((uint64_t)(kb >> 2) * 64u + lane) << 2) + (kb & 3u)]; };
        uint32_t steps = 0;
        stopped = walk_in_strip(fetch, s * rows, lgR, d.N, global, cy, cx, steps, nullptr);
        off = steps;
        const uint32_t ey = cy_start, ex = cx_start;
        while (!stopped && s > 0) {
            --s;
            uint32_t c_lo, c_hi;
            uint4 m = make_uint4(0, 0, 0, 2);
            const bool in_band = tb_band(ey, ex, cy, d.N, c_lo, c_hi) && cx >= c_lo && cx <= c_hi;
            if (in_band) m = a.map[(size_t)s * (d.N + 1) + cx];
            // .w: how this strip is crossed (ALN_TRACE_TB prints it; the segments kernel only asks whether it is 0) -- 2 = by its map
            // entry, 3 = entered outside the band, 4 = inside, but the map's walk had given up; 1 = the end cell's own strip
            a.seg[s] = make_uint4(cy, cx, off, m.w != 2u ? 2u : in_band ? 4u : 3u);
            if (m.w != 2u) {
                cx = m.x; cy = m.y; off += m.z; stopped = m.w != 0;
            } else {                                             // outside the band, or an entry the map gave up on: walk this strip here
                const uint32_t *wb = reinterpret_cast<const uint32_t *>(a.dirs + d.dir_off + s * aln_uniform_strip_bytes(d.N, a.R));
                auto fetch2 = [&](uint32_t kb, uint32_t lane) -> uint32_t { return wb[(((uint64_t)(kb >> 2) * 64u + lane) << 2) + (kb & 3u)]; };
                uint32_t st = 0;
                stopped = walk_in_strip(fetch2, s * rows, lgR, d.N, global, cy, cx, st, nullptr);
                off += st;
            }
        }
        if (!stopped && global && cy == 0 && cx != 0) {      // left strip 0 through the top border: D[0][x] = Left
            // (walk_in_strip handles the borders inside strip 0, so this cannot happen; kept as a guard)
            off += cx; cx = 0;
        }
    }
    res.start_y = cy; res.start_x = cx;
    res.aln_len = off + (a.pwm ? 0u : 1u);              // + the duplicated seed pair (none for the PWM aligner)
}

// one block per strip: stages the window its segment starts in, then one thread re-walks the segment and writes the
// tags at their final offset
extern "C" __global__ __launch_bounds__(256) void aln_tb_single_segments_kernel(TraceSingleArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem_words[];
    const uint32_t s = blockIdx.x;
    if (s >= a.ns) return;
    const PairDesc &d = a.descs[a.pair];
    if (a.results[a.pair].status != ALN_OK || (d.layout & 0xffu) != ALN_LAYOUT_UNIFORM) return;
    const uint4 sg = a.seg[s];
    if (sg.w == 0) return;
    const uint32_t lgR = 31u - (uint32_t)__builtin_clz(a.R), rows = 64u << lgR;
    const bool global = (a.semantics == ALN_CORE_GLOBAL || a.semantics == ALN_LEGACY_GLOBAL);
    uint8_t *ops = a.tags + d.tag_off + sg.z;
    const uint32_t *wbase = reinterpret_cast<const uint32_t *>(a.dirs + d.dir_off + s * aln_uniform_strip_bytes(d.N, a.R));
    uint32_t cy = sg.x, cx = sg.y, steps = 0;
    const uint32_t y0 = s * rows;
    const uint32_t k_hi = (cx ? cx - 1u : 0u) + ((cy > y0 ? cy - 1u - y0 : 0u) >> lgR);
    const StripWindow w = stage_window(wbase, smem_words, tb_window_quads(a.R), k_hi, lgR);
    const uint32_t q_lo = w.q_lo, q_n = w.q_n;
    // LDS through an address-space-3 pointer: a generic pointer would turn the two loads into one flat_load with a select
    const __attribute__((address_space(3))) uint32_t *lds3 = (const __attribute__((address_space(3))) uint32_t *)smem_words;
    auto fetch = [&](uint32_t kb, uint32_t lane) -> uint32_t {
        const uint32_t q = kb >> 2, rel = q - q_lo;
        uint32_t word = lds3[((min(rel, q_n - 1u) * 64u + lane) << 2) + (kb & 3u)];            // ds_read, always in range
        if (__builtin_expect(rel >= q_n, 0)) word = wbase[(((uint64_t)q * 64u + lane) << 2) + (kb & 3u)];   // left the window (rare)
        return word;
    };
    if (threadIdx.x == 0) walk_in_strip(fetch, y0, lgR, d.N, global, cy, cx, steps, ops);
}

// Pass 2 for one large pair: one block of 1024 threads (the per-pair wave of aln_traceback_expand_kernel would take
// ~100 us for 20 000 tags).  Same arithmetic: each thread sums its contiguous slice, block-wide exclusive scan, replay.
extern "C" __global__ __launch_bounds__(1024) void aln_tb_single_expand_kernel(TraceArgs a, uint32_t pair)
{
    __shared__ uint32_t wsum_y[16], wsum_x[16];
    const PairDesc &d = a.descs[pair];
    const aln_pair_result &res = a.results[pair];
    if (res.status != ALN_OK || (d.layout & 0xffu) != ALN_LAYOUT_UNIFORM) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint8_t *__restrict__ q = a.seqs + d.q_off;
    const uint8_t *__restrict__ t = a.seqs + d.t_off;
    const uint32_t cap = d.N + d.M + 2;
    uint8_t *__restrict__ qa = a.tb + d.tb_off;
    uint8_t *__restrict__ ta = qa + (a.pwm ? 4ull : 1ull) * cap;     // PWM: 4-byte column numbers instead of query residues (pwm/mod.rs:86-101)
    uint32_t *__restrict__ numbered = reinterpret_cast<uint32_t *>(qa);
    const uint8_t *__restrict__ ops = a.tags + d.tag_off;
    const uint32_t len = res.aln_len - (a.pwm ? 0u : 1u);
    const uint32_t per = (len + 1023u) / 1024u;
    const uint32_t lo = min(len, tid * per), hi = min(len, lo + per);
    uint32_t dy = 0, dx = 0;
    for (uint32_t j = lo; j < hi; ++j) {
        const uint32_t tag = ops[len - 1 - j];
        dx += (tag != 2u); dy += (tag != 1u);
    }
    uint32_t sy = dy, sx = dx;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const uint32_t oy = (uint32_t)__shfl_up((int)sy, m), ox = (uint32_t)__shfl_up((int)sx, m);
        if ((int)lane >= m) { sy += oy; sx += ox; }
    }
    if (lane == 63) { wsum_y[wave] = sy; wsum_x[wave] = sx; }
    __syncthreads();
    uint32_t by = 0, bx = 0;
    for (uint32_t wv = 0; wv < wave; ++wv) { by += wsum_y[wv]; bx += wsum_x[wv]; }
    uint32_t py = res.start_y + by + sy - dy, px = res.start_x + bx + sx - dx;
    for (uint32_t j = lo; j < hi; ++j) {
        const uint32_t tag = ops[len - 1 - j];
        px += (tag != 2u); py += (tag != 1u);
        if (a.pwm) numbered[j] = (tag == 2u) ? 0u : px;
        else qa[j] = (tag == 2u) ? a.blank : q[px - 1];
        ta[j] = (tag == 1u) ? a.blank : t[py - 1];
    }
    if (tid == 0 && !a.pwm) {
        qa[len] = q[res.end_x - 1];                     // the duplicated seed pair
        ta[len] = t[res.end_y - 1];
    }
}

// Pass 2, one wave per pair: turns the tag string into the two aligned code strings in final (forward) order.
// Position j of the output is step (len - 1 - j); its cell is the stop cell plus the moves of the steps after it, i.e.
// a prefix sum over the tags -- each lane sums its contiguous slice, one wave scan, then each lane replays its slice.
// 32 VGPRs (the attribute counts pairs): one wave of this kernel fits beside a full grid of the fill kernel (3 x 160 of a SIMD's
// 512 registers), so the strings of chunk i are written while chunk i+1 fills instead of waiting for a workgroup slot.
extern "C" __global__ __attribute__((amdgpu_flat_work_group_size(256, 256), amdgpu_num_vgpr(16))) void aln_traceback_expand_kernel(TraceArgs a)
{
    const uint32_t pair = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (pair >= a.n_pairs) return;
    constexpr int G = 2;
    const int lane = threadIdx.x & 63;
    const PairDesc &d = a.descs[pair];
    const aln_pair_result &res = a.results[pair];
    if (res.status != ALN_OK) return;
    if ((d.layout & 0xffu) == ALN_LAYOUT_UNIFORM) return;      // large pairs: aln_tb_single_expand_kernel
    const uint8_t *__restrict__ q = a.seqs + d.q_off;
    const uint8_t *__restrict__ t = a.seqs + d.t_off;
    const uint32_t cap = d.N + d.M + 2;
    uint8_t *__restrict__ qa = a.tb + d.tb_off;
    uint8_t *__restrict__ ta = qa + (a.pwm ? 4ull : 1ull) * cap;
    const uint8_t *__restrict__ ops = a.tags + d.tag_off;
    uint32_t *__restrict__ numbered = reinterpret_cast<uint32_t *>(qa);    // PWM: column numbers instead of query residues
    const uint32_t len = res.aln_len - (a.pwm ? 0u : 1u);
    // Position j reads ops[len - 1 - j] and needs the number of moves in x / y among positions 0..j: lane l takes position
    // j0 + l, so tags, residues and both strings move in coalesced lines, the prefix counts come from two ballots, and two
    // such groups are in flight at once -- the loads of a group do not depend on the group before (a lane-contiguous split
    // was one dependent byte load per position: 2 x 35 round trips per pair).
    uint32_t base_y = (uint32_t)__builtin_amdgcn_readfirstlane((int)res.start_y);
    uint32_t base_x = (uint32_t)__builtin_amdgcn_readfirstlane((int)res.start_x);
    for (uint32_t j0 = 0; j0 < len; j0 += 64u * G) {
        uint32_t tag[G], px[G], py[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const uint32_t j = j0 + 64u * u + (uint32_t)lane;
            tag[u] = (j < len) ? (uint32_t)ops[len - 1 - j] : 3u;      // 3: beyond the end, moves nothing
        }
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const bool fx = (tag[u] != 2u) && (tag[u] != 3u), fy = (tag[u] != 1u) && (tag[u] != 3u);
            const uint64_t bx = __ballot(fx), by = __ballot(fy);
            px[u] = base_x + __builtin_amdgcn_mbcnt_hi((uint32_t)(bx >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bx, 0u)) + (fx ? 1u : 0u);
            py[u] = base_y + __builtin_amdgcn_mbcnt_hi((uint32_t)(by >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)by, 0u)) + (fy ? 1u : 0u);
            base_x += (uint32_t)__popcll(bx); base_y += (uint32_t)__popcll(by);
        }
        uint32_t qv[G], tv[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {                                   // the cell this step left: (py, px)
            qv[u] = (tag[u] == 2u || tag[u] == 3u) ? (uint32_t)a.blank : (a.pwm ? px[u] : (uint32_t)q[px[u] - 1]);
            tv[u] = (tag[u] == 1u || tag[u] == 3u) ? (uint32_t)a.blank : (uint32_t)t[py[u] - 1];
        }
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const uint32_t j = j0 + 64u * u + (uint32_t)lane;
            if (j < len) {
                if (a.pwm) numbered[j] = (tag[u] == 2u) ? 0u : px[u];  // pwm/mod.rs:86-101
                else qa[j] = (uint8_t)qv[u];
                ta[j] = (uint8_t)tv[u];
            }
        }
    }
    if (lane == 0 && !a.pwm) {
        qa[len] = q[res.end_x - 1];                     // simple/mod.rs:102-105, :213-216: the duplicated seed
        ta[len] = t[res.end_y - 1];
    }
}

// (M+1)x(N+1) Direction bytes for one pair = AlignmentResult.direction_matrix
extern "C" __global__ void aln_unpack_directions_kernel(const uint8_t *dirs, const PairDesc *descs, uint32_t pair,
                                                        int semantics, uint8_t *out)
{
    const PairDesc d = descs[pair];
    const uint64_t total = (uint64_t)(d.M + 1) * (d.N + 1);
    const bool global = (semantics == ALN_CORE_GLOBAL || semantics == ALN_LEGACY_GLOBAL);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t y = (uint32_t)(i / (d.N + 1)), x = (uint32_t)(i % (d.N + 1));
        out[i] = (uint8_t)dir_at(dirs, d, global, y, x);
    }
}

// dyadic schemes filled by the integer kernels (aln_host.hip, call_init): both scores of every summary times 2^-k, exactly
extern "C" __global__ __launch_bounds__(256) void aln_scale_results_kernel(aln_pair_result *results, uint32_t n, double factor)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && results[i].status == ALN_OK) { results[i].f *= factor; results[i].score *= factor; }
}

// ---------------------------------------------------------------- launch helpers used by aln_host.hip (aln_launch.h)
extern "C" void aln_launch_traceback(const TraceArgs *a, hipStream_t s)
{
    const uint32_t grid = (a->n_pairs + 63) / 64;
    hipLaunchKernelGGL(aln_traceback_kernel, dim3(grid), dim3(64), 0, s, *a);
}
extern "C" void aln_launch_scale_results(aln_pair_result *results, uint32_t n, double factor, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_scale_results_kernel, dim3((n + 255) / 256), dim3(256), 0, s, results, n, factor);
}
extern "C" void aln_launch_traceback_wave(const TraceArgs *a, hipStream_t s)
{
    hipLaunchKernelGGL(aln_traceback_wave_kernel, dim3((a->n_pairs + 3) / 4), dim3(256), 0, s, *a);
}
extern "C" void aln_launch_traceback_overlap(const TraceArgs *a, uint32_t waves, hipStream_t s)
{
    hipLaunchKernelGGL(aln_delay_kernel, dim3(1), dim3(64), 0, s, 3000u);
    hipLaunchKernelGGL(aln_traceback_overlap_kernel, dim3(waves), dim3(64), 0, s, *a);
}
extern "C" void aln_launch_traceback_expand(const TraceArgs *a, hipStream_t s)
{
    hipLaunchKernelGGL(aln_traceback_expand_kernel, dim3((a->n_pairs + 3) / 4), dim3(256), 0, s, *a);
}
extern "C" void aln_launch_traceback_single(const TraceSingleArgs *a, uint32_t N, hipStream_t s)
{
    const uint32_t lds = tb_window_quads(a->R) * 1024u;
    (void)N;
    hipLaunchKernelGGL(aln_tb_single_maps_kernel, dim3(TB_BAND / 256u, a->ns), dim3(256), lds, s, *a);
    hipLaunchKernelGGL(aln_tb_single_chain_kernel, dim3(1), dim3(64), 0, s, *a);
    hipLaunchKernelGGL(aln_tb_single_segments_kernel, dim3(a->ns), dim3(256), lds, s, *a);
}
extern "C" void aln_launch_traceback_expand_single(const TraceArgs *a, uint32_t pair, hipStream_t s)
{
    hipLaunchKernelGGL(aln_tb_single_expand_kernel, dim3(1), dim3(1024), 0, s, *a, pair);
}
extern "C" void aln_launch_unpack(const uint8_t *dirs, const PairDesc *descs, uint32_t pair, int semantics, uint8_t *out,
                                  uint64_t cells, hipStream_t s)
{
    uint32_t grid = (uint32_t)((cells + 255) / 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(aln_unpack_directions_kernel, dim3(grid), dim3(256), 0, s, dirs, descs, pair, semantics, out);
}
// the code object's warm-up (aln_create): the attributes of one kernel load the unit without launching anything
extern "C" int aln_warm_tb(void)
{
    hipFuncAttributes attr;
    return (int)hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&aln_traceback_expand_kernel));
}
