// aln_report.hip -- device side of aln_seqset_held_report / aln_seqset_held_filter (include/aligner_hip.h): the columns of held hits'
// aligned strings, classed and counted where the strings lie.  aln_report_rules.h is the rule; this file is its wave64 form and the
// filter's selection.
//
//   report    one wave per listed hit, ALN_REPORT_WAVES hits per workgroup.  The workgroup first stages the scheme's bit table in LDS
//             (<= 1 KiB).  Lane l takes columns l, l + 64, ... of both strings: byte loads at consecutive addresses from held_tb +
//             tb_off and N + M + 2 bytes later.  The class of column j - 1, which the gap opens need, comes from lane l - 1; lane 0
//             takes it from lane 63 of the round before (nothing in front of column 0).  Eight counters per lane are folded by
//             cross-lane moves at distances 32 .. 1 and lane 0 writes the 40-byte record.  No atomics.
//   filter    aln_select.h over the device array of ALL held hits' reports: Keep is aln_report_keep with N, M of the held table,
//             Emit writes the position and, when asked for, the record -- tiles of 2048, ascending held order.
//
// Every store is a plain C++ store of a thread (vector memory instructions).
#include <hip/hip_runtime.h>

#include "aln_device.h"
#include "aln_launch.h"
#include "aln_report_rules.h"
#include "aln_select.h"

#define ALN_REPORT_WAVES 4u

__device__ inline aln_hit_report report_from_lane(const aln_hit_report &a, uint32_t w)
{
    aln_hit_report b = aln_report_empty(ALN_OK);      // (the fold adds the counts only)
    b.columns = __shfl_down(a.columns, w, 64);
    b.identical = __shfl_down(a.identical, w, 64);
    b.positive = __shfl_down(a.positive, w, 64);
    b.mismatch = __shfl_down(a.mismatch, w, 64);
    b.q_gap = __shfl_down(a.q_gap, w, 64);
    b.t_gap = __shfl_down(a.t_gap, w, 64);
    b.q_gap_open = __shfl_down(a.q_gap_open, w, 64);
    b.t_gap_open = __shfl_down(a.t_gap_open, w, 64);
    return b;
}

// listed entry k = held hit list[k] (k itself without a list); rep[k] its record.  bits: aln_report_words(rows, cols) <=
// ALN_REPORT_MAX_WORDS words
__global__ __launch_bounds__(64 * ALN_REPORT_WAVES) void aln_report_kernel(const HeldEntry *held, const aln_pair_result *res,
                                                                           const uint8_t *tb, const uint32_t *list, uint32_t n_list,
                                                                           uint32_t n_held, const uint32_t *bits, uint32_t rows,
                                                                           uint32_t cols, uint32_t blank, uint32_t flags, aln_hit_report *rep)
{
    __shared__ uint32_t table[ALN_REPORT_MAX_WORDS];
    const uint32_t words = aln_report_words(rows, cols);
    for (uint32_t w = threadIdx.x; w < words && w < ALN_REPORT_MAX_WORDS; w += 64u * ALN_REPORT_WAVES) table[w] = bits[w];
    __syncthreads();                                  // (the only barrier: a wave without a hit leaves after it)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t k = (uint64_t)blockIdx.x * ALN_REPORT_WAVES + (threadIdx.x >> 6);
    if (k >= n_list) return;
    const uint32_t h = list ? list[k] : (uint32_t)k;
    if (h >= n_held) return;                          // checked on the host; never read beyond the held hits
    const aln_pair_result r = res[h];
    aln_hit_report a = aln_report_empty(r.status);
    if (r.status == ALN_OK) {                         // (the same for every lane of the wave)
        const HeldEntry d = held[h];
        const uint32_t cap = d.N + d.M + 2u;
        const uint32_t len = r.aln_len < cap ? r.aln_len : cap;
        const uint32_t n = aln_report_columns(len, flags);
        const uint8_t *__restrict__ qs = tb + d.tb_off;
        const uint8_t *__restrict__ ts = qs + cap;
        uint32_t carry = ALN_REPORT_NONE;             // class of the column in front of this round's first
        for (uint64_t j0 = 0; j0 < n; j0 += 64u) {    // (every lane runs every round: the moves below are the whole wave's)
            const uint64_t j = j0 + lane;
            const uint32_t c = j < n ? aln_report_class_of(qs[j], ts[j], blank, table, rows, cols) : (uint32_t)ALN_REPORT_NONE;
            uint32_t prev = __shfl_up(c, 1, 64);
            if (lane == 0) prev = carry;
            carry = __shfl(c, 63, 64);
            if (j < n) aln_report_take(&a, c, prev);
        }
        for (uint32_t w = 32u; w >= 1u; w >>= 1) a = aln_report_fold(a, report_from_lane(a, w));
    }
    if (lane == 0) rep[k] = a;
}

// ---- the filter's selection (aln_select.h): held entry k is kept by its report and its sequences' lengths; kept entry k goes to
// place o: its position, and its record when asked for
struct ReportKeep {
    const aln_hit_report *rep;
    const HeldEntry *held;
    aln_hit_filter filter;
    __device__ bool operator()(uint64_t k) const { return aln_report_keep(rep[k], filter, held[k].N, held[k].M); }
};
struct ReportEmit {
    const aln_hit_report *rep;
    uint64_t cap;
    uint32_t *positions;
    aln_hit_report *out;
    __device__ void operator()(uint32_t o, uint64_t k) const
    {
        if (o < cap) { positions[o] = (uint32_t)k; if (out) out[o] = rep[k]; }
    }
};

extern "C" void aln_report_launch(const HeldEntry *held, const aln_pair_result *res, const uint8_t *tb, const uint32_t *list,
                                  uint32_t n_list, uint32_t n_held, const uint32_t *bits, uint32_t rows, uint32_t cols, uint32_t blank,
                                  uint32_t flags, aln_hit_report *rep, hipStream_t s)
{
    if (n_list) hipLaunchKernelGGL(aln_report_kernel, dim3(blocks_of(n_list, ALN_REPORT_WAVES)), dim3(64 * ALN_REPORT_WAVES), 0, s, held, res, tb,
                                   list, n_list, n_held, bits, rows, cols, blank, flags, rep);
}

// tile_count / tile_off: aln_seqset_tiles(n_held) words each; positions (and out, optional): cap entries; count[0]: the kept entries
extern "C" void aln_report_launch_filter(const aln_hit_report *rep, const HeldEntry *held, uint32_t n_held, const aln_hit_filter *filter,
                                         uint32_t *tile_count, uint32_t *tile_off, uint32_t *count, uint64_t cap, uint32_t *positions,
                                         aln_hit_report *out, hipStream_t s)
{
    aln_select_launch(ReportKeep{rep, held, *filter}, ReportEmit{rep, cap, positions, out}, n_held, tile_count, tile_off, count, s);
}
