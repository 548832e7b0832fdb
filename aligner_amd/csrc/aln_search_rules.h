// aln_search_rules.h -- the k best partners per record over a candidate list (aln_seqset_candidate_best,
// include/aligner_hip_search.h): the selection of aln_best_rules.h on a sparse list of a rectangle's pairs instead of the whole
// rectangle.  No HIP, so that the host, the kernels (aln_search.hip) and a CPU test driver cut a list the same way.
//
// Candidate, order and fold are aln_best_rules.h's, unchanged: an entry is selectable iff aln_best_candidate says so of its status, f
// and sequence numbers; a row keeps the first min(k, t_count) of its selectable entries under aln_best_before; lists are folded with
// aln_best_place.  The order is total, so neither the chunking nor the geometry below can show in the result.
//
// New here is the geometry.  L[0 .. C) is the resident candidate list: ascending pair numbers of a rectangle with T = t_count targets
// per row (C <= 0xFFFFFFF0).
//   row        entry i belongs to row L[i] / T; its target is t_first + L[i] % T, its query q_first + L[i] / T
//   row_first  row_first[r], r = 0 .. q_count, is the number of entries with L[i] < r * T (the product in uint64_t); row r's entries
//              are the positions row_first[r] .. row_first[r + 1] - 1, possibly none
//   chunk      positions c0 .. c0 + n - 1; it touches the rows L[c0] / T .. L[c0 + n - 1] / T, some of which may have no entry
//   piece      pieces are cut by list POSITION, not by row: piece p of the chunk is the positions c0 + 2048 p ..
//              min(c0 + 2048 (p + 1), c0 + n) - 1.  A piece usually holds many short rows; a long row spans several pieces
//   segment    a row's positions inside the chunk: the intersection of the row's range and the chunk
//   run        the run of row r in piece p is the intersection of the row's range, the piece and the chunk: a contiguous position
//              range.  The list ascends, so rows ascend with the position: sorting a piece by (row ascending, then aln_best_before)
//              leaves every run at the positions it already had, and no prefix sums or per-row piece tables are needed
// All of it in uint64_t.
#pragma once
#include <stdint.h>

#include "aln_best_rules.h"

#define ALN_SEARCH_PIECE ALN_BEST_PIECE
#define ALN_SEARCH_PAD_ROW 0xFFFFFFFFu            // the row of a piece's padding entries: after every real row (q_count < 2^32 - 16)

// row_first[r]: the entries of L[0 .. count) below r * t_count (a binary search: at most 33 steps)
ALN_BEST_HD inline uint64_t aln_search_row_first(const uint64_t *list, uint64_t count, uint64_t r, uint64_t t_count)
{
    const uint64_t bound = r * t_count;
    uint64_t lo = 0, hi = count;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (list[mid] < bound) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

ALN_BEST_HD inline uint64_t aln_search_row(uint64_t pair, uint64_t t_count) { return pair / t_count; }
ALN_BEST_HD inline uint64_t aln_search_column(uint64_t pair, uint64_t t_count) { return pair % t_count; }

// pieces of a chunk of n positions
ALN_BEST_HD inline uint64_t aln_search_pieces(uint64_t n) { return (n + ALN_SEARCH_PIECE - 1u) / ALN_SEARCH_PIECE; }

// piece p (0 .. pieces - 1) of the chunk (c0, n): its first position and its positions
ALN_BEST_HD inline void aln_search_piece(uint64_t c0, uint64_t n, uint64_t p, uint64_t *start, uint64_t *len)
{
    const uint64_t a = p * ALN_SEARCH_PIECE;
    *start = c0 + a;
    *len = n - a < ALN_SEARCH_PIECE ? n - a : ALN_SEARCH_PIECE;
}

// the segment of a row with the range first .. next - 1 (row_first[r], row_first[r + 1]) in the chunk (c0, n): its first position,
// its positions (0: the row has no entry in the chunk, and the rest is not written), the first piece it overlaps and how many
ALN_BEST_HD inline uint64_t aln_search_row_segment(uint64_t first, uint64_t next, uint64_t c0, uint64_t n, uint64_t *start, uint64_t *piece0,
                                                   uint64_t *n_pieces)
{
    const uint64_t a = first > c0 ? first : c0, b = next < c0 + n ? next : c0 + n;
    if (b <= a) return 0;
    *start = a;
    *piece0 = (a - c0) / ALN_SEARCH_PIECE;
    *n_pieces = (b - 1u - c0) / ALN_SEARCH_PIECE - *piece0 + 1u;
    return b - a;
}

// the run of a segment (start, len: aln_search_row_segment, len >= 1) in piece p, one of the pieces it overlaps: first position, positions
ALN_BEST_HD inline void aln_search_run(uint64_t seg_start, uint64_t seg_len, uint64_t c0, uint64_t p, uint64_t *start, uint64_t *len)
{
    const uint64_t p0 = c0 + p * ALN_SEARCH_PIECE, p1 = p0 + ALN_SEARCH_PIECE;
    const uint64_t a = seg_start > p0 ? seg_start : p0, b = seg_start + seg_len < p1 ? seg_start + seg_len : p1;
    *start = a;
    *len = b - a;
}

// the first position of the run that holds position `at` of the chunk (c0, n), `at` being an entry of the row that starts at `first`
ALN_BEST_HD inline uint64_t aln_search_run_start(uint64_t first, uint64_t c0, uint64_t at)
{
    const uint64_t p0 = c0 + (at - c0) / ALN_SEARCH_PIECE * ALN_SEARCH_PIECE;
    return first > p0 ? first : p0;
}
