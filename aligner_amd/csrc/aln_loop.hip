// aln_loop.hip -- device side of the heuristic loop's step (aln_pairset_loop_begin / aln_pairset_loop_step, include/aligner_hip.h): what
// stands between a held run of a pair set and the next run's going list.
//
//   classify   entry k of the held run (pair going[k]) against that pair's resident best f, by aln_loop_rules.h: finished (done or
//              failed) or improved; an improved pair's best becomes its f
//   settle     an improved entry's class once the transform kernel (aln_pairset.hip) has answered: going, or finished without a root
//   select     the entries of one kind -- improved, going, finished -- compacted in ascending entry order by the shared two-level
//              prefix sum (aln_select.h): a predicate on the class and an emitter here.  The same lists every run, no atomic appends.
//              improved: pair numbers and held entries (what the transform kernel reads); going: the next step's list of pair numbers
//              (what the pick kernel reads); finished: pair numbers, causes and the 48-byte summaries, packed for one download
//
// Every store is a plain C++ store of a thread (vector memory instructions).
#include <hip/hip_runtime.h>

#include "aln_device.h"
#include "aln_launch.h"
#include "aln_loop_rules.h"
#include "aln_select.h"

// the kinds of a selection
#define LOOP_SEL_IMPROVED 0u
#define LOOP_SEL_GOING 1u
#define LOOP_SEL_FINISHED 2u

// ---- entry k of the held run: pair going[k], its summary res[k]
__global__ __launch_bounds__(256) void aln_loop_classify_kernel(const aln_pair_result *res, const uint32_t *going, uint32_t n, double *best,
                                                                uint32_t *cls)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t pair = going[k];
    const int32_t status = res[k].status;
    const double f = res[k].f;
    const uint32_t c = aln_loop_classify(status, f, best[pair]);
    if (c == ALN_LOOP_IMPROVED) best[pair] = f;          // a pair is listed once: no other thread reads or writes this word
    cls[k] = c;
}

// ---- listed transform c (held entry entry[c]; c itself without a table): going, or finished without a root
__global__ __launch_bounds__(256) void aln_loop_settle_kernel(const uint32_t *entry, const int32_t *transform_status, uint32_t n, uint32_t *cls)
{
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    cls[entry ? entry[c] : (uint32_t)c] = aln_loop_after_transform(transform_status[c]);
}

__device__ __forceinline__ bool loop_keep(uint32_t cls, uint32_t kind)
{
    return kind == LOOP_SEL_IMPROVED ? cls == ALN_LOOP_IMPROVED : kind == LOOP_SEL_GOING ? cls == ALN_LOOP_GOING : aln_loop_is_finished(cls);
}

// ---- selection (aln_select.h): entry k is kept by its class.  Kept entry k goes to place o: out_pair[o] = going[k] (k itself without
// a list); out_word[o] = k for the improved, the class (the cause) otherwise; out_res[o] = res[k] where asked for.  The outputs hold n
// entries: every entry may be kept.
struct LoopKeep {
    const uint32_t *cls;
    uint32_t kind;
    __device__ bool operator()(uint64_t k) const { return loop_keep(cls[k], kind); }
};
struct LoopEmit {
    const uint32_t *cls;
    uint32_t n, kind;
    const uint32_t *going;
    const aln_pair_result *res;
    uint32_t *out_pair, *out_word;
    aln_pair_result *out_res;
    __device__ void operator()(uint32_t o, uint64_t k) const
    {
        if (o < n) {
            out_pair[o] = going ? going[k] : (uint32_t)k;
            if (out_word) out_word[o] = kind == LOOP_SEL_IMPROVED ? (uint32_t)k : cls[k];
            if (out_res) out_res[o] = res[k];
        }
    }
};

extern "C" void aln_loop_launch_classify(const aln_pair_result *res, const uint32_t *going, uint32_t n, double *best, uint32_t *cls, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_loop_classify_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, res, going, n, best, cls);
}

extern "C" void aln_loop_launch_settle(const uint32_t *entry, const int32_t *transform_status, uint32_t n, uint32_t *cls, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_loop_settle_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, entry, transform_status, n, cls);
}

extern "C" uint32_t aln_loop_tiles(uint32_t n) { return (uint32_t)aln_select_tiles(n); }

// tile_count / tile_off: aln_loop_tiles(n) words each; count[0]: the kept entries; kind: 0 improved, 1 going, 2 finished
extern "C" void aln_loop_launch_select(const uint32_t *cls, uint32_t n, uint32_t kind, const uint32_t *going, const aln_pair_result *res,
                                       uint32_t *tile_count, uint32_t *tile_off, uint32_t *count, uint32_t *out_pair, uint32_t *out_word,
                                       aln_pair_result *out_res, hipStream_t s)
{
    aln_select_launch(LoopKeep{cls, kind}, LoopEmit{cls, n, kind, going, res, out_pair, out_word, out_res}, n, tile_count, tile_off, count, s);
}
