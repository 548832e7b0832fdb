// aln_cigar.hip -- device side of aln_seqset_held_cigar_plan / _fill (include/aligner_hip_cigar.h): the aligned strings of held hits
// run-length encoded where they lie.  aln_cigar_rules.h is the rule; this file is its wave64 form.
//
// the plan
//   count     one wave per listed hit, ALN_CIGAR_WAVES hits per workgroup, in the shape of aln_report_kernel.  Lane l takes columns l,
//             l + 64, ... of both strings.  A column is a run start iff its op differs from the op of the column in front of it, which
//             comes from lane l - 1; lane 0 takes it from lane 63 of the round before (ALN_CIGAR_NO_OP in front of column 0).  The runs,
//             the query and target non-blanks, the matches and the P columns are popcounts of 64-bit ballots, the same in every lane;
//             lane 0 stores the record and adds to the summary's counters
//   offsets   tile b = listed hits b * 256 .. : each thread's n_ops scanned within the tile (off[k] gets the place in the tile) and the
//             tile's sum; one workgroup turns the tile sums into tile offsets, 256 tiles a trip with a 64-bit carry, as
//             aln_select_offsets_kernel does for 32-bit counts; a last pass adds each tile's offset and writes off[n] = the total.
//             256 records of up to 2^28 words pass 32 bits, so the sums are 64-bit: aln_block_exclusive_scan runs once per 16-bit limb
//             of the values (each limb's block sum stays below 2^24) and the limbs' results are added up in 64 bits
// the fill (buffers only; nothing is decided again)
//   write     the same walk, one wave per listed hit.  Only a run's last column writes: the next column's op comes from lane l + 1 and
//             for lane 63 from one look-ahead load of column j + 1, guarded by j + 1 < n, so the seed column is never read.  The run's
//             index is the run starts at or below the column (this round's ballot plus a count carried across rounds) minus one; its
//             length is j - s + 1, s the highest run-start bit at or below the lane, else a second carried value: the start of the run
//             that was open when the round began, so a run across one or more rounds is one word.  Lane 0 writes the clips.
//             A stranded plan (aln_seqset_held_strand_cigar_plan) marks the listed hits whose target is a mirror: their word r goes
//             to place n_ops - 1 - r of the hit's words, clips included; nothing else differs and a plain plan has no marks
//
// Bounds: a column index stays below aln_len clipped to N + M + 2, the room of one string in the held store (the look-ahead load too);
// a listed position is compared with n_held before it indexes; a word index is compared with off[k + 1] and with the plan's total
// before every store.  Atomics: integer adds of the summary's counters only.  Every op word is a plain C++ store of exactly one thread.
// No kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include "aln_cigar_rules.h"
#include "aln_device.h"
#include "aln_launch.h"
#include "aln_select.h"
#include "aln_strand_rules.h"

#define ALN_CIGAR_WAVES 4u
static_assert(ALN_CIGAR_TILE == ALN_SELECT_THREADS, "a tile is one value per thread of the block scan");

// the strings of listed hit k, the same for every lane of the wave
struct CigarHit {
    const uint8_t *qs, *ts;
    uint32_t n, N;               // counted columns; the query's length
    uint32_t start_x, start_y;
    int32_t status;
    bool listed;                 // the position is one of the held hits
};
__device__ __forceinline__ CigarHit aln_cigar_hit(const CigarArgs &a, uint64_t k)
{
    CigarHit m;
    m.qs = m.ts = nullptr; m.n = 0; m.N = 0; m.start_x = m.start_y = 0; m.status = ALN_ERR_INVALID_ARGUMENT;
    const uint32_t h = a.list[k];
    m.listed = h < a.n_held;                          // (checked on the host; never read beyond the held hits)
    if (!m.listed) return m;
    const aln_pair_result r = a.res[h];
    m.status = r.status;
    if (r.status != ALN_OK) return m;
    const HeldEntry d = a.held[h];
    const uint32_t cap = d.N + d.M + 2u;
    const uint32_t len = r.aln_len < cap ? r.aln_len : cap;
    m.qs = a.tb + d.tb_off;
    m.ts = m.qs + cap;
    m.n = aln_cigar_columns(len);
    m.N = d.N;
    m.start_x = r.start_x; m.start_y = r.start_y;
    return m;
}

__global__ __launch_bounds__(64 * ALN_CIGAR_WAVES) void aln_cigar_count_kernel(CigarArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t k = (uint64_t)blockIdx.x * ALN_CIGAR_WAVES + (threadIdx.x >> 6);
    if (k >= a.n_list) return;
    const CigarHit m = aln_cigar_hit(a, k);
    if (m.status != ALN_OK) {                         // (the same for every lane of the wave)
        if (lane == 0) {
            a.rec[k] = aln_cigar_empty(m.status);
            atomicAdd(&a.misc[ALN_CIGAR_MISC_FAILED], 1ull);
        }
        return;
    }
    uint32_t runs = 0, q_res = 0, t_res = 0, matches = 0, pads = 0;
    uint32_t carry = ALN_CIGAR_NO_OP;                 // the op of the column in front of this round's first
    for (uint64_t j0 = 0; j0 < m.n; j0 += 64u) {      // (every lane runs every round: the ballots are the whole wave's)
        const uint64_t j = j0 + lane;
        const bool in = j < m.n;
        const uint32_t x = in ? m.qs[j] : a.blank, y = in ? m.ts[j] : a.blank;
        const uint32_t op = in ? aln_cigar_op(x, y, a.blank, a.flags) : ALN_CIGAR_NO_OP;
        uint32_t prev = __shfl_up(op, 1, 64);
        if (lane == 0) prev = carry;
        carry = __shfl(op, 63, 64);
        runs += (uint32_t)__popcll(__ballot(in && op != prev));
        q_res += (uint32_t)__popcll(__ballot(in && x != a.blank));
        t_res += (uint32_t)__popcll(__ballot(in && y != a.blank));
        matches += (uint32_t)__popcll(__ballot(in && x == y && x != a.blank));
        pads += (uint32_t)__popcll(__ballot(in && op == ALN_CIGAR_P));
    }
    if (lane == 0) {
        const aln_cigar_record r = aln_cigar_finish(runs, q_res, t_res, matches, pads, m.n, m.start_x, m.start_y, m.N, a.flags);
        a.rec[k] = r;
        if (pads) atomicAdd(&a.misc[ALN_CIGAR_MISC_PADDED], (unsigned long long)pads);
        if (aln_cigar_overflows(r.q_end, m.N, a.flags)) atomicAdd(&a.misc[ALN_CIGAR_MISC_OVERFLOW], 1ull);
    }
}

// block-wide exclusive prefix sum of one value below 2^48 per thread (256 threads), exact in 64 bits: aln_block_exclusive_scan over
// the value's three 16-bit limbs, whose block sums stay below 2^24
__device__ __forceinline__ uint64_t aln_cigar_scan(uint64_t v, uint32_t *lds, uint64_t *total)
{
    uint64_t ex = 0, sum = 0;
    for (uint32_t limb = 0; limb < 3u; ++limb) {
        uint32_t t;
        const uint32_t e = aln_block_exclusive_scan((uint32_t)(v >> (16u * limb)) & 0xFFFFu, lds, &t);
        ex += (uint64_t)e << (16u * limb);
        sum += (uint64_t)t << (16u * limb);
    }
    *total = sum;
    return ex;
}

__global__ __launch_bounds__(256) void aln_cigar_tile_kernel(CigarArgs a)
{
    __shared__ uint32_t lds[ALN_SELECT_THREADS];
    const uint64_t k = (uint64_t)blockIdx.x * ALN_SELECT_THREADS + threadIdx.x;
    const uint64_t v = k < a.n_list ? a.rec[k].n_ops : 0u;
    uint64_t total;
    const uint64_t ex = aln_cigar_scan(v, lds, &total);
    if (k < a.n_list) a.off[k] = ex;
    if (threadIdx.x == 0 && blockIdx.x < a.tiles) a.tile_sum[blockIdx.x] = total;
}

// the like of aln_select_offsets_kernel for 64-bit tile sums (each below 2^37: 256 records of less than 2^29 words)
__global__ __launch_bounds__(256) void aln_cigar_tile_offsets_kernel(CigarArgs a)
{
    __shared__ uint32_t lds[ALN_SELECT_THREADS];
    uint64_t carry = 0;
    for (uint64_t b = 0; b < a.tiles; b += ALN_SELECT_THREADS) {
        const uint64_t i = b + threadIdx.x;
        const uint64_t v = i < a.tiles ? a.tile_sum[i] : 0ull;
        uint64_t trip;
        const uint64_t ex = aln_cigar_scan(v, lds, &trip);
        if (i < a.tiles) a.tile_off[i] = carry + ex;
        carry += trip;
    }
    if (threadIdx.x == 0) {
        a.misc[ALN_CIGAR_MISC_TOTAL] = carry;
        a.off[a.n_list] = carry;                      // (off has n_list + 1 entries)
    }
}

__global__ __launch_bounds__(256) void aln_cigar_offsets_kernel(CigarArgs a)
{
    const uint64_t k = (uint64_t)blockIdx.x * ALN_SELECT_THREADS + threadIdx.x;
    if (k < a.n_list && blockIdx.x < a.tiles) a.off[k] += a.tile_off[blockIdx.x];
}

// ---- the fill
__global__ __launch_bounds__(64 * ALN_CIGAR_WAVES) void aln_cigar_write_kernel(CigarArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t k = (uint64_t)blockIdx.x * ALN_CIGAR_WAVES + (threadIdx.x >> 6);
    if (k >= a.n_list) return;
    const aln_cigar_record rec = a.rec[k];
    if (rec.status != ALN_OK || rec.n_ops == 0u) return;
    const CigarHit m = aln_cigar_hit(a, k);
    if (m.status != ALN_OK) return;
    const uint64_t first = a.off[k], end = a.off[k + 1u];
    const bool reversed = a.rev && a.rev[k];          // (a stranded plan's hit on a mirrored target: aln_strand_rules.h)
    auto put = [&](uint64_t w, uint64_t length, uint32_t op) {
        if (reversed) w = first + aln_strand_word_pos(w - first, rec.n_ops, true);
        if (w >= first && w < end && w < a.total) a.ops[w] = aln_cigar_word(length, op);
    };
    const uint32_t lead = aln_cigar_lead(rec.q_start, a.flags), trail = aln_cigar_trail(rec.q_end, m.N, a.flags);
    if (lane == 0) {
        if (lead) put(first, lead, ALN_CIGAR_S);
        if (trail) put(first + rec.n_ops - 1u, trail, ALN_CIGAR_S);
    }
    const uint64_t base = first + (lead ? 1u : 0u);
    uint32_t carry = ALN_CIGAR_NO_OP;                 // the op of the column in front of this round's first
    uint64_t before = 0;                              // run starts in the rounds before this one
    uint64_t open = 0;                                // the first column of the run that was open when this round began
    for (uint64_t j0 = 0; j0 < m.n; j0 += 64u) {      // (every lane runs every round: the ballot and the moves are the whole wave's)
        const uint64_t j = j0 + lane;
        const bool in = j < m.n;
        const uint32_t op = in ? aln_cigar_op(m.qs[j], m.ts[j], a.blank, a.flags) : ALN_CIGAR_NO_OP;
        uint32_t prev = __shfl_up(op, 1, 64);
        if (lane == 0) prev = carry;
        carry = __shfl(op, 63, 64);
        uint32_t next = __shfl_down(op, 1, 64);
        if (lane == 63u) next = j + 1u < m.n ? aln_cigar_op(m.qs[j + 1u], m.ts[j + 1u], a.blank, a.flags) : ALN_CIGAR_NO_OP;
        const unsigned long long starts = __ballot(in && op != prev);
        const unsigned long long upto = starts & ((2ull << lane) - 1ull);          // the run starts at or below this lane
        if (in && next != op) {                       // a run's last column
            const uint64_t s = upto ? j0 + (uint64_t)(63 - __clzll((long long)upto)) : open;
            const uint64_t index = before + (uint64_t)__popcll(upto) - 1ull;       // (column 0 is a run start: never 0 - 1)
            put(base + index, j - s + 1ull, op);
        }
        before += (uint64_t)__popcll(starts);
        if (starts) open = j0 + (uint64_t)(63 - __clzll((long long)starts));
    }
}

extern "C" int aln_warm_cigar(void)
{
    hipFuncAttributes attr;
    hipError_t e = hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&aln_cigar_count_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&aln_cigar_write_kernel));
    return (int)e;
}

// misc zeroed before; rec, off (n_list + 1), tile_sum and tile_off (tiles = aln_cigar_tiles(n_list) each) are written
extern "C" void aln_cigar_launch_plan(const CigarArgs *a, hipStream_t s)
{
    if (a->n_list) hipLaunchKernelGGL(aln_cigar_count_kernel, dim3(blocks_of(a->n_list, ALN_CIGAR_WAVES)), dim3(64 * ALN_CIGAR_WAVES), 0, s, *a);
    if (a->tiles) hipLaunchKernelGGL(aln_cigar_tile_kernel, dim3((uint32_t)a->tiles), dim3(ALN_SELECT_THREADS), 0, s, *a);
    hipLaunchKernelGGL(aln_cigar_tile_offsets_kernel, dim3(1), dim3(ALN_SELECT_THREADS), 0, s, *a);
    if (a->tiles) hipLaunchKernelGGL(aln_cigar_offsets_kernel, dim3((uint32_t)a->tiles), dim3(ALN_SELECT_THREADS), 0, s, *a);
}

// ops: `total` words
extern "C" void aln_cigar_launch_fill(const CigarArgs *a, hipStream_t s)
{
    if (a->n_list && a->total) hipLaunchKernelGGL(aln_cigar_write_kernel, dim3(blocks_of(a->n_list, ALN_CIGAR_WAVES)), dim3(64 * ALN_CIGAR_WAVES), 0, s, *a);
}
