// aln_msa.hip -- device side of aln_seqset_held_msa_plan / _fill (include/aligner_hip_msa.h): the held hits of every centre merged into
// one set of columns, centre-star, where the strings lie.  aln_msa_rules.h is the rule; this file is its wave64 form.
//
// the plan
//   slots     one thread per centre: slot_of[centers[i]] = i (the table was filled with ALN_CLUSTER_NONE on the stream before) and record
//             i gets its centre; the other words of the records, ins and misc were zeroed on the stream before
//   measure   one wave per held hit, ALN_MSA_WAVES hits per workgroup; the decision is aln_profile_kernel's.  A hit that does not
//             contribute stores ALN_CLUSTER_NONE into mark[h] and adds one to its counter from lane 0; a contributing hit stores its slot
//             and adds one to rows[slot].  Lane l takes columns l, l + 64, ... of the centre's string.  `before` of a column is a base
//             carried from round to round plus the popcount of the ballot "centre non-blank" below the lane; the column of the last
//             centre non-blank in front of a column is the highest bit of that ballot below the lane, else a second carried value,
//             so a run of blanks that crosses a round is one run.  Only a run's last column (the next column is no counted blank: one
//             more byte load) issues atomicMax(&ins[slot][p], run length)
//   layout    one workgroup per centre: col[p] = p + ins[0] + ... + ins[p] by aln_block_exclusive_scan over trips of 256 positions with
//             a 64-bit carry, then width and inserted of the record (a width beyond 32 bits: saturated and counted)
// the fill (buffers only; nothing is decided again)
//   centre    one workgroup per centre: row 0 (the output was filled with the blank code on the stream before) and its row-list entry
//   tickets   a thread per held hit with a mark: t = atomicAdd(&taken[slot], 1), list[slot][t] = h
//   rank      one wave per held hit with a mark: the entries of its family's list below h, counted by ballot and popcount in strides
//             of 64.  row = 1 + rank; the held positions are distinct, so the rows do not depend on the order of the tickets.
//             O(rows^2) per family
//   write     one wave per row walks the hit's strings as measure did and stores each counted member code at its column
//
// Bounds: a column index stays below aln_len clipped to N + M + 2, the room of one string in the held store (the look-ahead byte of a
// run's end too: j + 1 < n); a position is compared with len[centre] in 64 bits before it indexes ins / col; slot_of is indexed with a
// sequence number below n_seqs only; a slot is compared with n_centers, a ticket with rows, a row with rows + 1, a column with the
// width and a byte offset with the capacity before they index.  Atomics: integer max and add only.  Every (row, column) is written by
// exactly one thread; every store is a plain C++ store of a thread.  No kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include "aln_device.h"
#include "aln_launch.h"
#include "aln_msa_rules.h"
#include "aln_select.h"

#define ALN_MSA_WAVES 4u
#define ALN_MSA_THREADS 256u

__global__ __launch_bounds__(256) void aln_msa_slots_kernel(const uint32_t *centers, uint32_t n_centers, uint32_t n_seqs, uint32_t *slot_of, aln_msa_record *rec)
{
    const uint64_t i = (uint64_t)blockIdx.x * ALN_MSA_THREADS + threadIdx.x;
    if (i >= n_centers) return;
    const uint32_t c = centers[i];
    rec[i].center = c;
    if (c < n_seqs) slot_of[c] = (uint32_t)i;         // (checked on the host; never written beyond the table)
}

// what measure and write share: the strings of a contributing hit and where its centre lies
struct MsaHit {
    const uint8_t *cs, *ms;      // the centre's and the member's aligned string
    uint32_t n, start, len_c;    // counted columns, the centre's start coordinate and length
};
__device__ __forceinline__ MsaHit aln_msa_hit(const MsaArgs &a, uint64_t h, uint32_t c, bool c_is_q)
{
    const aln_pair_result r = a.res[h];
    const HeldEntry d = a.held[h];
    const uint32_t cap = d.N + d.M + 2u;
    const uint32_t len = r.aln_len < cap ? r.aln_len : cap;
    const uint8_t *qs = a.tb + d.tb_off;
    const uint8_t *ts = qs + cap;
    MsaHit m;
    m.cs = c_is_q ? qs : ts;
    m.ms = c_is_q ? ts : qs;
    m.n = aln_msa_columns(len);
    m.start = c_is_q ? r.start_x : r.start_y;
    m.len_c = a.len[c];
    return m;
}

// one round of 64 columns: what lane `lane` knows of column j0 + lane afterwards
struct MsaColumn {
    bool in, residue;            // a counted column; its centre code is not blank
    uint32_t before;             // centre non-blanks in front of it
    uint32_t run;                // centre blank: the column's number in its run, from 0
};
__device__ __forceinline__ MsaColumn aln_msa_round(const MsaHit &m, uint64_t j0, uint32_t lane, uint32_t blank, uint32_t &base, int64_t &last)
{
    const uint64_t j = j0 + lane;
    MsaColumn c;
    c.in = j < m.n;
    c.residue = c.in && m.cs[j] != blank;
    const unsigned long long mask = __ballot(c.residue);
    const unsigned long long below = mask & ((1ull << lane) - 1ull);
    c.before = base + (uint32_t)__popcll(below);
    const int64_t prev = below ? (int64_t)j0 + (63 - __clzll((long long)below)) : last;       // the last centre non-blank in front, -1: none
    c.run = (uint32_t)((int64_t)j - prev - 1);
    base += (uint32_t)__popcll(mask);
    if (mask) last = (int64_t)j0 + (63 - __clzll((long long)mask));
    return c;
}

__global__ __launch_bounds__(64 * ALN_MSA_WAVES) void aln_msa_measure_kernel(MsaArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t h = (uint64_t)blockIdx.x * ALN_MSA_WAVES + (threadIdx.x >> 6);
    if (h >= a.n_held) return;
    // (everything up to the loop is the same for every lane of the wave)
    uint32_t c = 0, c_is_q = 0, slot = ALN_CLUSTER_NONE;
    uint32_t kind = ALN_PROFILE_SKIP;
    const aln_pair_result r = a.res[h];
    const uint32_t q = a.hit_q[h], t = a.hit_t[h];
    if (r.status == ALN_OK && q < a.n_seqs && t < a.n_seqs) {       // (the endpoints were checked on the host; never indexed beyond)
        const HeldEntry d = a.held[h];
        if (!a.rep || aln_report_keep(a.rep[h], a.filter, d.N, d.M)) kind = aln_profile_decide(q, t, a.label[q], a.label[t], &c, &c_is_q);
    }
    if (kind == ALN_PROFILE_COUNTS) {
        slot = c < a.n_seqs ? a.slot_of[c] : ALN_CLUSTER_NONE;        // (c is q or t)
        if (slot >= a.n_centers) kind = ALN_PROFILE_UNLISTED;
    }
    if (kind != ALN_PROFILE_COUNTS) {
        if (lane == 0) {
            a.mark[h] = ALN_CLUSTER_NONE;
            if (kind != ALN_PROFILE_SKIP) atomicAdd(&a.misc[kind], 1ull);
        }
        return;
    }
    const MsaHit m = aln_msa_hit(a, h, c, c_is_q != 0);
    const uint64_t first = a.ins_off[slot];
    uint32_t base = 0, over = 0;
    int64_t last = -1;
    for (uint64_t j0 = 0; j0 < m.n; j0 += 64u) {       // (every lane runs every round: the ballot is the whole wave's)
        const MsaColumn k = aln_msa_round(m, j0, lane, a.blank, base, last);
        if (!k.in) continue;
        const uint64_t p = aln_msa_position(m.start, k.before);
        if (k.residue) {
            over += aln_msa_residue_fits(p, m.len_c) ? 0u : 1u;
        } else if (!aln_msa_insert_fits(p, m.len_c)) {
            over += 1u;
        } else {
            const uint64_t j = j0 + lane;
            const bool ends = j + 1u >= m.n || m.cs[j + 1u] != a.blank;
            if (ends && first + p < a.n_ins) atomicMax(&a.ins[first + p], k.run + 1u);
        }
    }
    for (uint32_t w = 32u; w >= 1u; w >>= 1) over += __shfl_down(over, w, 64);
    if (lane == 0) {
        a.mark[h] = slot;
        atomicAdd(&a.rec[slot].rows, 1u);
        atomicAdd(&a.misc[ALN_PROFILE_COUNTS], 1ull);
        if (over) atomicAdd(&a.misc[ALN_PROFILE_MISC_OVERFLOW], (unsigned long long)over);
    }
}

__global__ __launch_bounds__(256) void aln_msa_layout_kernel(MsaArgs a)
{
    __shared__ uint32_t lds[ALN_SELECT_THREADS];
    const uint32_t slot = blockIdx.x;
    if (slot >= a.n_centers) return;
    const uint32_t c = a.rec[slot].center;
    const uint32_t len_c = c < a.n_seqs ? a.len[c] : 0u;
    const uint64_t first = a.ins_off[slot], entries = (uint64_t)len_c + 1ull;
    uint64_t carry = 0;
    for (uint64_t b = 0; b < entries; b += ALN_SELECT_THREADS) {
        const uint64_t p = b + threadIdx.x;
        const bool in = p < entries && first + p < a.n_ins;
        const uint32_t v = in ? a.ins[first + p] : 0u;
        uint32_t trip;
        const uint32_t ex = aln_block_exclusive_scan(v, lds, &trip);
        if (in) a.col[first + p] = (uint32_t)(p + carry + ex + v);      // (meaningless beyond 32 bits: the plan is refused then)
        carry += trip;
    }
    if (threadIdx.x == 0) {
        const uint64_t width = (uint64_t)len_c + carry;
        const bool fits = width <= 0xFFFFFFFFull;
        a.rec[slot].width = fits ? (uint32_t)width : 0xFFFFFFFFu;
        a.rec[slot].inserted = fits ? (uint32_t)carry : 0xFFFFFFFFu - len_c;
        if (!fits) atomicAdd(&a.misc[ALN_MSA_MISC_TOO_WIDE], 1ull);
    }
}

// ---- the fill
__global__ __launch_bounds__(256) void aln_msa_center_kernel(MsaArgs a)
{
    const uint32_t slot = blockIdx.x;
    if (slot >= a.n_centers) return;
    const aln_msa_record rec = a.rec[slot];
    const uint32_t c = rec.center;
    if (c >= a.n_seqs) return;
    const uint32_t len_c = a.len[c];
    const uint64_t first = a.ins_off[slot], at = a.byte_off[slot];
    const uint8_t *residues = a.seqs + a.seq_off[c];
    for (uint64_t p = threadIdx.x; p < len_c; p += ALN_MSA_THREADS) {
        if (first + p >= a.n_ins) break;
        const uint32_t col = a.col[first + p];
        if (col < rec.width && at + col < a.bytes) a.out[at + col] = residues[p];
    }
    if (threadIdx.x == 0 && a.row_off[slot] < a.total_rows) a.row_hit[a.row_off[slot]] = ALN_CLUSTER_NONE;
}

__global__ __launch_bounds__(256) void aln_msa_ticket_kernel(MsaArgs a)
{
    const uint64_t h = (uint64_t)blockIdx.x * ALN_MSA_THREADS + threadIdx.x;
    if (h >= a.n_held) return;
    const uint32_t slot = a.mark[h];
    if (slot >= a.n_centers) return;
    const uint32_t t = atomicAdd(&a.taken[slot], 1u);
    const uint64_t at = a.row_off[slot] + 1ull + t;
    if (t < a.rec[slot].rows && at < a.total_rows) a.list[at] = (uint32_t)h;
}

__global__ __launch_bounds__(64 * ALN_MSA_WAVES) void aln_msa_rank_kernel(MsaArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t h = (uint64_t)blockIdx.x * ALN_MSA_WAVES + (threadIdx.x >> 6);
    if (h >= a.n_held) return;
    const uint32_t slot = a.mark[h];
    if (slot >= a.n_centers) {
        if (lane == 0) a.hit_row[h] = ALN_CLUSTER_NONE;
        return;
    }
    const uint32_t rows = a.rec[slot].rows;
    const uint64_t first = a.row_off[slot] + 1ull;
    uint32_t rank = 0;
    for (uint64_t i0 = 0; i0 < rows; i0 += 64u) {      // (every lane runs every round)
        const uint64_t i = i0 + lane;
        const bool below = i < rows && first + i < a.total_rows && a.list[first + i] < (uint32_t)h;
        rank += (uint32_t)__popcll(__ballot(below));
    }
    if (lane == 0) {
        const uint32_t row = 1u + rank;
        const bool ok = row <= rows && a.row_off[slot] + row < a.total_rows;
        a.hit_row[h] = ok ? row : ALN_CLUSTER_NONE;
        if (ok) a.row_hit[a.row_off[slot] + row] = (uint32_t)h;
    }
}

__global__ __launch_bounds__(64 * ALN_MSA_WAVES) void aln_msa_write_kernel(MsaArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t h = (uint64_t)blockIdx.x * ALN_MSA_WAVES + (threadIdx.x >> 6);
    if (h >= a.n_held) return;
    const uint32_t slot = a.mark[h];
    if (slot >= a.n_centers) return;
    const aln_msa_record rec = a.rec[slot];
    const uint32_t row = a.hit_row[h];
    if (row == 0u || row > rec.rows) return;
    const uint32_t c = rec.center;
    if (c >= a.n_seqs) return;
    const MsaHit m = aln_msa_hit(a, h, c, a.hit_q[h] == c);
    const uint64_t first = a.ins_off[slot];
    const uint64_t at = a.byte_off[slot] + (uint64_t)row * rec.width;
    uint32_t base = 0;
    int64_t last = -1;
    for (uint64_t j0 = 0; j0 < m.n; j0 += 64u) {       // (every lane runs every round: the ballot is the whole wave's)
        const MsaColumn k = aln_msa_round(m, j0, lane, a.blank, base, last);
        if (!k.in) continue;
        const uint64_t p = aln_msa_position(m.start, k.before);
        if (!(k.residue ? aln_msa_residue_fits(p, m.len_c) : aln_msa_insert_fits(p, m.len_c)) || first + p >= a.n_ins) continue;
        uint64_t col = a.col[first + p];
        if (!k.residue) {
            const uint32_t wide = a.ins[first + p];
            if (k.run >= wide) continue;
            col = aln_msa_insert_column((uint32_t)col, wide, k.run);
        }
        if (col < rec.width && at + col < a.bytes) a.out[at + col] = m.ms[j0 + lane];
    }
}

extern "C" int aln_warm_msa(void)
{
    hipFuncAttributes attr;
    hipError_t e = hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&aln_msa_measure_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&aln_msa_write_kernel));
    return (int)e;
}

// slot_of: n_seqs words, filled with ALN_CLUSTER_NONE before; rec, ins and misc zeroed before.  mark gets a word for every held hit
extern "C" void aln_msa_launch_plan(const MsaArgs *a, const uint32_t *centers, uint32_t *slot_of, hipStream_t s)
{
    if (a->n_centers)
        hipLaunchKernelGGL(aln_msa_slots_kernel, dim3(blocks_of(a->n_centers, ALN_MSA_THREADS)), dim3(ALN_MSA_THREADS), 0, s, centers, a->n_centers, a->n_seqs,
                           slot_of, a->rec);
    if (a->n_held)                                    // (without centres too: the summary's counters are the kernel's)
        hipLaunchKernelGGL(aln_msa_measure_kernel, dim3(blocks_of(a->n_held, ALN_MSA_WAVES)), dim3(64 * ALN_MSA_WAVES), 0, s, *a);
    if (a->n_centers) hipLaunchKernelGGL(aln_msa_layout_kernel, dim3(a->n_centers), dim3(ALN_MSA_THREADS), 0, s, *a);
}

// out filled with the blank code and taken zeroed before
extern "C" void aln_msa_launch_fill(const MsaArgs *a, hipStream_t s)
{
    if (a->n_centers) hipLaunchKernelGGL(aln_msa_center_kernel, dim3(a->n_centers), dim3(ALN_MSA_THREADS), 0, s, *a);
    if (!a->n_held || !a->n_centers) return;
    hipLaunchKernelGGL(aln_msa_ticket_kernel, dim3(blocks_of(a->n_held, ALN_MSA_THREADS)), dim3(ALN_MSA_THREADS), 0, s, *a);
    hipLaunchKernelGGL(aln_msa_rank_kernel, dim3(blocks_of(a->n_held, ALN_MSA_WAVES)), dim3(64 * ALN_MSA_WAVES), 0, s, *a);
    hipLaunchKernelGGL(aln_msa_write_kernel, dim3(blocks_of(a->n_held, ALN_MSA_WAVES)), dim3(64 * ALN_MSA_WAVES), 0, s, *a);
}
