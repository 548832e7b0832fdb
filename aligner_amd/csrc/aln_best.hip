// aln_best.hip -- device side of aln_seqset_best (include/aligner_hip.h): the k best targets of every query row of a rectangle of a
// resident sequence set, selected where the scores are.  The rule -- candidate, order, geometry, fold -- is aln_best_rules.h.
//
//   piece      one workgroup per (touched row, piece of <= 2048 pairs) of a chunk: the candidates' (key, target) go into LDS (2048 x 12
//              bytes), non-candidates as a sentinel that sorts last; a bitonic sort under the rule; the first min(slots, candidates)
//              go out to the chunk's candidate buffer
//   merge      one wave per touched row: the row's piece lists, each sorted, are folded one after the other into the row's running list
//              (rank by counting over <= 2 x 64 entries per fold).  A row cut by a chunk border meets its running list again in the next
//              chunk; the launches of one stream keep the order
//   finish     after the last chunk: rows' counts -> tile sums (256 rows per tile, one row per thread), the shared scan over the tiles
//              with 64-bit offsets (aln_select.h), then every tile writes its rows' entries in ascending target order at their
//              offsets: one ascending (pair number, f) list, no atomics
//
// Every loop is bounded by the problem size, no kernel waits for another workgroup, every store is a plain C++ store.
#include <hip/hip_runtime.h>

#include "aln_best_rules.h"
#include "aln_launch.h"
#include "aln_select.h"

#define BEST_THREADS 256u
#define BEST_TILE_ROWS ALN_SELECT_THREADS            // one row per thread of the block scan
#define BEST_SENTINEL_T 0xFFFFFFFFu               // with key 0 (no candidate has it): after every candidate

// ---- piece p of the chunk: sorted, its first min(slots, candidates) at cand_*[p * slots ..], their number in cand_n[p]
__global__ __launch_bounds__(256) void aln_best_piece_kernel(const double *f, const int32_t *status, uint64_t n, uint64_t k0, uint64_t t_count,
                                                             uint64_t q_first, uint64_t t_first, double f_min, uint32_t flags, uint32_t slots,
                                                             uint64_t *cand_key, uint32_t *cand_t, uint32_t *cand_n)
{
    __shared__ uint64_t s_key[ALN_BEST_PIECE];
    __shared__ uint32_t s_t[ALN_BEST_PIECE];
    const aln_best_chunk g = aln_best_chunk_geometry(k0, n, t_count);
    const uint64_t p = blockIdx.x;
    if (p >= g.pieces) return;
    uint64_t j, start, len;
    aln_best_piece(g, t_count, p, &j, &start, &len);
    uint32_t N = 1;                                // the sort's size: len <= 2048 rounded up to a power of two
    while (N < len) N <<= 1;
    const uint64_t q = q_first + g.row0 + j;
    const uint64_t t0 = t_first + (k0 + start) % t_count;        // a piece lies within one row
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < N; i += BEST_THREADS) {
        uint64_t key = 0;
        uint32_t t = BEST_SENTINEL_T;
        if (i < len) {
            const uint64_t at = start + i;         // < n
            const double v = f[at];
            if (aln_best_candidate(status[at], v, f_min, q, t0 + i, flags)) { key = aln_best_key(v); t = (uint32_t)(t0 + i); }
        }
        s_key[i] = key;
        s_t[i] = t;
    }
    __syncthreads();
    for (uint32_t size = 2; size <= N; size <<= 1)
        for (uint32_t stride = size >> 1; stride; stride >>= 1) {
            for (uint32_t i = tid; i < N / 2u; i += BEST_THREADS) {
                const uint32_t lo = 2u * i - (i & (stride - 1u)), hi = lo + stride;
                const bool first_best = (lo & size) == 0u;       // the last pass (size == N) runs in this direction throughout
                const uint64_t ka = s_key[lo], kb = s_key[hi];
                const uint32_t ta = s_t[lo], tb = s_t[hi];
                const bool swap = first_best ? aln_best_before(kb, tb, ka, ta) : aln_best_before(ka, ta, kb, tb);
                if (swap) { s_key[lo] = kb; s_t[lo] = tb; s_key[hi] = ka; s_t[hi] = ta; }
            }
            __syncthreads();
        }
    const uint32_t top = slots < N ? slots : N;    // <= 64
    if (tid < top) {
        const bool have = s_key[tid] != 0;
        if (have) { cand_key[p * slots + tid] = s_key[tid]; cand_t[p * slots + tid] = s_t[tid]; }
        const bool more = tid + 1u < top && s_key[tid + 1u] != 0;
        if (have && !more) cand_n[p] = tid + 1u;
        if (!have && tid == 0) cand_n[p] = 0;
    }
}

// ---- touched row j of the chunk: its piece lists folded into run_*[row * slots ..] / run_n[row]
__global__ __launch_bounds__(64) void aln_best_merge_kernel(uint64_t n, uint64_t k0, uint64_t t_count, uint32_t slots, const uint64_t *cand_key,
                                                            const uint32_t *cand_t, const uint32_t *cand_n, uint64_t *run_key, uint32_t *run_t,
                                                            uint32_t *run_n)
{
    __shared__ uint64_t a_key[ALN_SEQSET_BEST_MAX], b_key[ALN_SEQSET_BEST_MAX];
    __shared__ uint32_t a_t[ALN_SEQSET_BEST_MAX], b_t[ALN_SEQSET_BEST_MAX];
    const aln_best_chunk g = aln_best_chunk_geometry(k0, n, t_count);
    const uint64_t j = blockIdx.x;
    if (j >= g.rows) return;
    uint64_t start, len, piece0, n_pieces;
    aln_best_row_segment(g, t_count, j, &start, &len, &piece0, &n_pieces);
    const uint64_t row = g.row0 + j;
    const uint32_t lane = threadIdx.x;
    uint32_t na = run_n[row];
    if (na > slots) na = slots;
    if (lane < na) { a_key[lane] = run_key[row * slots + lane]; a_t[lane] = run_t[row * slots + lane]; }
    for (uint64_t p = piece0; p < piece0 + n_pieces; ++p) {
        uint32_t nb = cand_n[p];
        if (nb > slots) nb = slots;
        if (lane < nb) { b_key[lane] = cand_key[p * slots + lane]; b_t[lane] = cand_t[p * slots + lane]; }
        __syncthreads();
        uint64_t ka = 0, kb = 0;
        uint32_t ta = 0, tb = 0, pa = slots, pb = slots;
        if (lane < na) { ka = a_key[lane]; ta = a_t[lane]; pa = aln_best_place(lane, ka, ta, b_key, b_t, nb); }
        if (lane < nb) { kb = b_key[lane]; tb = b_t[lane]; pb = aln_best_place(lane, kb, tb, a_key, a_t, na); }
        __syncthreads();
        if (pa < slots) { a_key[pa] = ka; a_t[pa] = ta; }
        if (pb < slots) { a_key[pb] = kb; a_t[pb] = tb; }
        na = na + nb < slots ? na + nb : slots;
        __syncthreads();
    }
    if (lane < na) { run_key[row * slots + lane] = a_key[lane]; run_t[row * slots + lane] = a_t[lane]; }
    if (lane == 0) run_n[row] = na;
}

// ---- finish, step 1: kept entries per tile of 256 rows
__global__ __launch_bounds__(256) void aln_best_count_kernel(const uint32_t *run_n, uint64_t rows, uint32_t *tile_count)
{
    __shared__ uint32_t lds[ALN_SELECT_THREADS];
    const uint64_t row = (uint64_t)blockIdx.x * BEST_TILE_ROWS + threadIdx.x;
    uint32_t total;
    (void)aln_block_exclusive_scan(row < rows ? run_n[row] : 0u, lds, &total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// ---- finish, step 3: a tile's rows, each in ascending target order (rank by counting within the row; one wave per row, four rows
// at a time), at the tile's offset plus the row's: pair number in the block and f
__global__ __launch_bounds__(256) void aln_best_emit_kernel(const uint64_t *run_key, const uint32_t *run_t, const uint32_t *run_n, uint64_t rows,
                                                            uint32_t slots, uint64_t t_count, uint64_t t_first, const uint64_t *tile_off,
                                                            uint64_t cap, uint64_t *out_k, double *out_f)
{
    __shared__ uint32_t lds[ALN_SELECT_THREADS];
    __shared__ uint32_t row_off[BEST_TILE_ROWS];
    const uint64_t row0 = (uint64_t)blockIdx.x * BEST_TILE_ROWS;
    const uint64_t mine = row0 + threadIdx.x;
    uint32_t total;
    row_off[threadIdx.x] = aln_block_exclusive_scan(mine < rows ? run_n[mine] : 0u, lds, &total);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = tile_off[blockIdx.x];
    for (uint32_t r = wave; r < BEST_TILE_ROWS; r += BEST_THREADS / 64u) {
        const uint64_t row = row0 + r;
        if (row >= rows) break;
        uint32_t nr = run_n[row];
        if (nr > slots) nr = slots;
        if (lane >= nr) continue;
        const uint32_t *ts = run_t + row * slots;
        const uint32_t t = ts[lane];
        uint32_t rank = 0;
        for (uint32_t i = 0; i < nr; ++i) rank += ts[i] < t ? 1u : 0u;
        const uint64_t o = base + row_off[r] + rank;
        if (o < cap) { out_k[o] = row * t_count + (t - t_first); out_f[o] = aln_best_unkey(run_key[row * slots + lane]); }
    }
}

extern "C" int aln_warm_best(void)
{
    hipFuncAttributes attr;
    return (int)hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&aln_best_piece_kernel));
}

// one chunk: f / status of its n pairs (pair numbers k0 .. k0 + n - 1 of the rectangle) -> the running lists of the rows it touches.
// cand_key / cand_t: aln_best_chunk_geometry(k0, n, t_count).pieces * slots entries; cand_n: one word per piece
extern "C" void aln_best_launch_chunk(const double *f, const int32_t *status, uint64_t n, uint64_t k0, const aln_seqset_block *block,
                                      double f_min, uint32_t flags, uint32_t slots, uint64_t *cand_key, uint32_t *cand_t, uint32_t *cand_n,
                                      uint64_t *run_key, uint32_t *run_t, uint32_t *run_n, hipStream_t s)
{
    if (!n) return;
    const aln_best_chunk g = aln_best_chunk_geometry(k0, n, block->t_count);
    hipLaunchKernelGGL(aln_best_piece_kernel, dim3((uint32_t)g.pieces), dim3(BEST_THREADS), 0, s, f, status, n, k0, block->t_count,
                       block->q_first, block->t_first, f_min, flags, slots, cand_key, cand_t, cand_n);
    hipLaunchKernelGGL(aln_best_merge_kernel, dim3((uint32_t)g.rows), dim3(64), 0, s, n, k0, block->t_count, slots, cand_key, cand_t, cand_n,
                       run_key, run_t, run_n);
}

extern "C" uint64_t aln_best_tiles(uint64_t rows) { return (rows + BEST_TILE_ROWS - 1) / BEST_TILE_ROWS; }

// tile_count: aln_best_tiles(rows) words, each <= 256 x 64; tile_off: as many uint64_t (2^32 rows of 64); total[0]: the kept entries of
// all rows
extern "C" void aln_best_launch_count(const uint32_t *run_n, uint64_t rows, uint32_t *tile_count, uint64_t *tile_off, uint64_t *total, hipStream_t s)
{
    const uint64_t tiles = aln_best_tiles(rows);
    if (tiles) hipLaunchKernelGGL(aln_best_count_kernel, dim3((uint32_t)tiles), dim3(BEST_THREADS), 0, s, run_n, rows, tile_count);
    hipLaunchKernelGGL(aln_select_offsets_kernel<uint64_t>, dim3(1), dim3(ALN_SELECT_THREADS), 0, s, tile_count, tile_off, tiles, total);
}

// out_k / out_f: cap entries (the total of aln_best_launch_count)
extern "C" void aln_best_launch_emit(const uint64_t *run_key, const uint32_t *run_t, const uint32_t *run_n, uint64_t rows, uint32_t slots,
                                     const aln_seqset_block *block, const uint64_t *tile_off, uint64_t cap, uint64_t *out_k, double *out_f,
                                     hipStream_t s)
{
    const uint64_t tiles = aln_best_tiles(rows);
    if (tiles && cap) hipLaunchKernelGGL(aln_best_emit_kernel, dim3((uint32_t)tiles), dim3(BEST_THREADS), 0, s, run_key, run_t, run_n, rows, slots,
                                         block->t_count, block->t_first, tile_off, cap, out_k, out_f);
}
