// aln_search.hip -- device side of aln_seqset_candidate_best (include/aligner_hip_search.h): the k best targets of every query row
// among the pairs of a resident candidate list, selected where the scores are.  Candidate, order and fold are aln_best_rules.h's; the
// geometry of a sparse list -- rows found by position, pieces cut by position -- is aln_search_rules.h.
//
//   rows       once per call: row_first[r] for r = 0 .. q_count, one thread and one binary search in the list each
//   piece      one workgroup per piece of <= 2048 list positions of a chunk: every entry's (row, key, target) goes into LDS (2048 x 16
//              bytes), a non-selectable entry with key 0 and the sentinel target, so that it sorts last within its row; a bitonic sort
//              under (row ascending, then the rule's order).  The list ascends, so every run of a row stays at the positions it had:
//              the sorted (key, target) go back to the chunk's buffer at their chunk positions, the first `slots` of each run
//   merge      one wave per touched row: the leading entries of the row's runs, piece after piece, are folded into the row's running
//              list (rank by counting over <= 2 x 64 entries per fold, as aln_best_merge_kernel does).  A row cut by a chunk border
//              meets its running list again in the next chunk; the launches of one stream keep the order
//   finish     aln_best.hip's count, scan and emit, unchanged
//
// Every loop is bounded by the problem size, no kernel waits for another workgroup, every store is a plain C++ store.
#include <hip/hip_runtime.h>

#include "aln_search_rules.h"
#include "aln_launch.h"

#define SEARCH_THREADS 256u
#define SEARCH_SENTINEL_T 0xFFFFFFFFu             // with key 0 (no selectable entry has it): after every selectable entry of the row

struct SearchEntry { uint64_t key; uint32_t t; uint32_t row; };      // 16 bytes

__device__ inline bool search_before(const SearchEntry &a, const SearchEntry &b)
{
    return a.row < b.row || (a.row == b.row && aln_best_before(a.key, a.t, b.key, b.t));
}

// ---- row_first[r] = entries of the list below r * t_count, r = 0 .. q_count
__global__ __launch_bounds__(256) void aln_search_rows_kernel(const uint64_t *list, uint64_t count, uint64_t q_count, uint64_t t_count,
                                                              uint32_t *row_first)
{
    const uint64_t r = (uint64_t)blockIdx.x * SEARCH_THREADS + threadIdx.x;
    if (r > q_count) return;
    row_first[r] = (uint32_t)aln_search_row_first(list, count, r, t_count);         // (count <= 0xFFFFFFF0)
}

// ---- piece p of the chunk (c0, n): sorted by (row, order); the first `slots` of every run at piece_*[position - c0].  f / status are
// indexed by chunk position, list and row_first by list position and row
__global__ __launch_bounds__(256) void aln_search_piece_kernel(const uint64_t *list, const uint32_t *row_first, const double *f, const int32_t *status,
                                                               uint64_t c0, uint64_t n, uint64_t t_count, uint64_t q_first, uint64_t t_first,
                                                               double f_min, uint32_t flags, uint32_t slots, uint64_t *piece_key, uint32_t *piece_t)
{
    __shared__ SearchEntry s_e[ALN_SEARCH_PIECE];
    const uint64_t p = blockIdx.x;
    if (p >= aln_search_pieces(n)) return;
    uint64_t start, len;
    aln_search_piece(c0, n, p, &start, &len);
    uint32_t N = 1;                                // the sort's size: len <= 2048 rounded up to a power of two
    while (N < len) N <<= 1;
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < N; i += SEARCH_THREADS) {
        SearchEntry e;
        e.key = 0; e.t = SEARCH_SENTINEL_T; e.row = ALN_SEARCH_PAD_ROW;
        if (i < len) {
            const uint64_t pair = list[start + i];                 // start + i < c0 + n
            const uint64_t row = aln_search_row(pair, t_count), t = t_first + aln_search_column(pair, t_count);
            const uint64_t at = start - c0 + i;                     // < n
            const double v = f[at];
            e.row = (uint32_t)row;
            if (aln_best_candidate(status[at], v, f_min, q_first + row, t, flags)) { e.key = aln_best_key(v); e.t = (uint32_t)t; }
        }
        s_e[i] = e;
    }
    __syncthreads();
    for (uint32_t size = 2; size <= N; size <<= 1)
        for (uint32_t stride = size >> 1; stride; stride >>= 1) {
            for (uint32_t i = tid; i < N / 2u; i += SEARCH_THREADS) {
                const uint32_t lo = 2u * i - (i & (stride - 1u)), hi = lo + stride;
                const bool first_best = (lo & size) == 0u;       // the last pass (size == N) runs in this direction throughout
                const SearchEntry a = s_e[lo], b = s_e[hi];
                const bool swap = first_best ? search_before(b, a) : search_before(a, b);
                if (swap) { s_e[lo] = b; s_e[hi] = a; }
            }
            __syncthreads();
        }
    for (uint32_t i = tid; i < len; i += SEARCH_THREADS) {
        const SearchEntry e = s_e[i];                  // (a real entry: the padding sorts after all of them)
        const uint64_t at = start + i;
        if (at - aln_search_run_start(row_first[e.row], c0, at) < slots) { piece_key[at - c0] = e.key; piece_t[at - c0] = e.t; }
    }
}

// ---- touched row row0 + blockIdx.x of the chunk: the leading entries of its runs folded into run_*[row * slots ..] / run_n[row]
__global__ __launch_bounds__(64) void aln_search_merge_kernel(const uint32_t *row_first, uint64_t c0, uint64_t n, uint64_t row0, uint64_t rows,
                                                              uint32_t slots, const uint64_t *piece_key, const uint32_t *piece_t, uint64_t *run_key,
                                                              uint32_t *run_t, uint32_t *run_n)
{
    __shared__ uint64_t a_key[ALN_SEQSET_BEST_MAX], b_key[ALN_SEQSET_BEST_MAX];
    __shared__ uint32_t a_t[ALN_SEQSET_BEST_MAX], b_t[ALN_SEQSET_BEST_MAX];
    if (blockIdx.x >= rows) return;
    const uint64_t row = row0 + blockIdx.x;
    uint64_t seg, piece0 = 0, n_pieces = 0;
    const uint64_t seg_len = aln_search_row_segment(row_first[row], row_first[row + 1u], c0, n, &seg, &piece0, &n_pieces);
    if (!seg_len) return;                              // a row between two others, without an entry in the chunk
    const uint32_t lane = threadIdx.x;
    uint32_t na = run_n[row];
    if (na > slots) na = slots;
    if (lane < na) { a_key[lane] = run_key[row * slots + lane]; a_t[lane] = run_t[row * slots + lane]; }
    for (uint64_t p = piece0; p < piece0 + n_pieces; ++p) {
        uint64_t rs, rl;
        aln_search_run(seg, seg_len, c0, p, &rs, &rl);
        const uint32_t m = rl < slots ? (uint32_t)rl : slots;
        b_key[lane] = lane < m ? piece_key[rs - c0 + lane] : 0;
        b_t[lane] = lane < m ? piece_t[rs - c0 + lane] : SEARCH_SENTINEL_T;
        __syncthreads();
        uint32_t nb = 0;                               // the run's selectable entries lead it: up to the first key 0
        while (nb < m && b_key[nb] != 0) ++nb;
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

extern "C" int aln_warm_search(void)
{
    hipFuncAttributes attr;
    return (int)hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&aln_search_piece_kernel));
}

// row_first: q_count + 1 words
extern "C" void aln_search_launch_rows(const uint64_t *list, uint64_t count, uint64_t q_count, uint64_t t_count, uint32_t *row_first, hipStream_t s)
{
    const uint64_t blocks = (q_count + 1u + SEARCH_THREADS - 1u) / SEARCH_THREADS;
    hipLaunchKernelGGL(aln_search_rows_kernel, dim3((uint32_t)blocks), dim3(SEARCH_THREADS), 0, s, list, count, q_count, t_count, row_first);
}

// one chunk: f / status of list positions c0 .. c0 + n - 1 -> the running lists of the rows row0 .. row0 + rows - 1 it touches.
// piece_key / piece_t: n entries
extern "C" void aln_search_launch_chunk(const uint64_t *list, const uint32_t *row_first, const double *f, const int32_t *status, uint64_t c0, uint64_t n,
                                        uint64_t row0, uint64_t rows, const aln_seqset_block *block, double f_min, uint32_t flags, uint32_t slots,
                                        uint64_t *piece_key, uint32_t *piece_t, uint64_t *run_key, uint32_t *run_t, uint32_t *run_n, hipStream_t s)
{
    if (!n || !rows) return;
    hipLaunchKernelGGL(aln_search_piece_kernel, dim3((uint32_t)aln_search_pieces(n)), dim3(SEARCH_THREADS), 0, s, list, row_first, f, status, c0, n,
                       block->t_count, block->q_first, block->t_first, f_min, flags, slots, piece_key, piece_t);
    hipLaunchKernelGGL(aln_search_merge_kernel, dim3((uint32_t)rows), dim3(64), 0, s, row_first, c0, n, row0, rows, slots, piece_key, piece_t,
                       run_key, run_t, run_n);
}
