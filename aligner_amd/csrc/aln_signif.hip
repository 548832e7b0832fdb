// aln_signif.hip -- device side of aln_seqset_held_significance (include/aligner_hip.h): what the shuffled copies of a chunk's hits
// leave behind.  The copies themselves are aln_shuffle.hip's (drawn from per-hit streams) and the fill is the batch's; this file
// holds the reduction of their 48-byte summaries into one aln_signif_record per hit, in the order of aln_signif_rules.h.
//
//   reduce    one wave per hit, ALN_SIGNIF_WAVES hits per workgroup.  Lane l is accumulator l of the rule: it reads the summaries of
//             copies l, l + 64, ... (f and status of each) in ascending order, then the 64 accumulators are folded by cross-lane moves
//             at distances 32, 16, 8, 4, 2, 1 -- lane l < w keeps a[l] (+) a[l + w], the rule's order -- and lane 0 writes the record.
//             No atomics, no LDS.  The per-copy f is written only when the caller asked for it.
//
// Every store is a plain C++ store of a thread (vector memory instructions).
#include <hip/hip_runtime.h>

#include "aln_device.h"
#include "aln_launch.h"
#include "aln_signif_rules.h"

#define ALN_SIGNIF_WAVES 4u

static_assert(ALN_SIGNIF_LANES == 64u, "one lane per accumulator of the rule: wave64");

__device__ inline aln_signif_record signif_from_lane(const aln_signif_record &a, uint32_t w)
{
    aln_signif_record b;
    b.sum = __shfl_down(a.sum, w, 64);
    b.sum_sq = __shfl_down(a.sum_sq, w, 64);
    b.f_max = __shfl_down(a.f_max, w, 64);
    b.n_ok = __shfl_down(a.n_ok, w, 64);
    b.n_ge = __shfl_down(a.n_ge, w, 64);
    b.status = __shfl_down(a.status, w, 64);
    b.first_bad = __shfl_down(a.first_bad, w, 64);
    return b;
}

// hit h of the chunk: the summaries of its copies at res[h * per_pair ..), its held score f_hit[h]; rec[h] its record; f (optional):
// f[h * per_pair + s] the f of copy s
__global__ __launch_bounds__(64 * ALN_SIGNIF_WAVES) void aln_signif_reduce_kernel(const aln_pair_result *res, const double *f_hit,
                                                                                  uint32_t n_hits, uint32_t per_pair,
                                                                                  aln_signif_record *rec, double *f)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t h = (uint64_t)blockIdx.x * ALN_SIGNIF_WAVES + (threadIdx.x >> 6);
    if (h >= n_hits) return;                         // (the whole wave leaves: no barrier follows)
    const aln_pair_result *r = res + h * per_pair;
    double *fo = f ? f + h * per_pair : nullptr;
    const double hit = f_hit[h];
    aln_signif_record a = aln_signif_empty();
    for (uint32_t s = lane; s < per_pair; s += ALN_SIGNIF_LANES) {
        const double v = r[s].f;
        const int32_t st = r[s].status;
        if (fo) fo[s] = v;
        aln_signif_take(&a, s, v, st, hit);
    }
    // (lanes at or above w fold as well: what they then hold is never read by a lane below the next w)
    for (uint32_t w = ALN_SIGNIF_LANES / 2; w >= 1u; w >>= 1) a = aln_signif_fold(a, signif_from_lane(a, w));
    if (lane == 0) rec[h] = a;
}

extern "C" void aln_signif_launch_reduce(const aln_pair_result *res, const double *f_hit, uint32_t n_hits, uint32_t per_pair,
                                         aln_signif_record *rec, double *f, hipStream_t s)
{
    if (n_hits) hipLaunchKernelGGL(aln_signif_reduce_kernel, dim3(blocks_of(n_hits, ALN_SIGNIF_WAVES)), dim3(64 * ALN_SIGNIF_WAVES), 0, s, res,
                                   f_hit, n_hits, per_pair, rec, f);
}
