// aln_best_rules.h -- the k best targets per query of a rectangle of a resident sequence set (aln_seqset_best, include/aligner_hip.h):
// who is a candidate, which of two candidates comes first, how a chunk of consecutive pair numbers is cut into rows and pieces, and
// how two sorted lists of one row are folded into one.  No HIP, so that the host, the kernels (aln_best.hip) and a CPU test driver
// decide all four the same way.
//
//   candidate  a pair of the row with status ALN_OK, f == f and f >= f_min (plain IEEE compares: a NaN on either side selects
//              nothing); with ALN_BEST_SKIP_SELF also q != t as sequence numbers
//   order      (f, t) comes before (f', t') iff f > f', or f == f' and t < t'.  -0.0 == +0.0.  The kernels compare integers: the key
//              of f is monotone in f with -0.0 folded onto +0.0, so (key, t) before (key', t') iff key > key', or key == key' and
//              t < t'.  The targets of a row are distinct, so the order is total and a row's k best are one fixed set, whatever
//              the launch geometry, the chunking or the order of arrival
//   geometry   a chunk is the pair numbers k0 .. k0 + n - 1 of a rectangle with t_count targets per query.  It touches the rows
//              k0 / t_count .. (k0 + n - 1) / t_count; the first and the last of them may be cut, the rows between them are whole.
//              A row's segment is cut into pieces of at most ALN_BEST_PIECE pairs, counted from the segment's first pair.  Pieces are
//              numbered row by row.  All of it in uint64_t: k0 may lie beyond 2^32
//   fold       two lists of one row, each sorted under the order, -> the first `cap` of their union, sorted: an entry's place is its
//              own index plus the number of entries of the other list that come before it (rank by counting; no entry of one list
//              equals one of the other: their targets differ)
#pragma once
#include <stdint.h>

#include "../../include/aligner_hip.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define ALN_BEST_HD __host__ __device__
#else
#define ALN_BEST_HD
#endif

#define ALN_BEST_PIECE 2048u                      // the tile of the set's selection (aln_seqset.hip)

// monotone key: f < g <=> key(f) < key(g) for all non-NaN f, g; key(-0.0) == key(+0.0).  No non-NaN f has key 0.
ALN_BEST_HD inline uint64_t aln_best_key(double f)
{
    uint64_t b;
    __builtin_memcpy(&b, &f, 8);
    if (b == 0x8000000000000000ull) b = 0;        // -0.0 -> +0.0
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// the f of a key (a folded zero comes back as +0.0)
ALN_BEST_HD inline double aln_best_unkey(uint64_t key)
{
    const uint64_t b = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
    double f;
    __builtin_memcpy(&f, &b, 8);
    return f;
}

ALN_BEST_HD inline bool aln_best_candidate(int32_t status, double f, double f_min, uint64_t q, uint64_t t, uint32_t flags)
{
    if (status != ALN_OK || !(f == f) || !(f >= f_min)) return false;
    return !((flags & ALN_BEST_SKIP_SELF) && q == t);
}

ALN_BEST_HD inline bool aln_best_before(uint64_t key_a, uint32_t t_a, uint64_t key_b, uint32_t t_b)
{
    return key_a > key_b || (key_a == key_b && t_a < t_b);
}

// ---- geometry of a chunk (n >= 1, t_count >= 1)
struct aln_best_chunk {
    uint64_t row0;            // first touched row (query index within the block)
    uint64_t rows;            // touched rows
    uint64_t len_first;       // pairs of the first touched row inside the chunk
    uint64_t len_last;        // pairs of the last touched row inside the chunk (== len_first if rows == 1)
    uint64_t p_first, p_full, p_last;   // pieces of the first row's segment, of a whole row, of the last row's segment
    uint64_t pieces;          // all pieces of the chunk
};

ALN_BEST_HD inline uint64_t aln_best_pieces_of(uint64_t len) { return (len + ALN_BEST_PIECE - 1u) / ALN_BEST_PIECE; }

ALN_BEST_HD inline aln_best_chunk aln_best_chunk_geometry(uint64_t k0, uint64_t n, uint64_t t_count)
{
    aln_best_chunk g;
    const uint64_t last = k0 + (n - 1u);
    g.row0 = k0 / t_count;
    g.rows = last / t_count - g.row0 + 1u;
    const uint64_t c0 = k0 % t_count;
    g.len_first = g.rows == 1u ? n : t_count - c0;
    g.len_last = g.rows == 1u ? n : last % t_count + 1u;
    g.p_first = aln_best_pieces_of(g.len_first);
    g.p_full = aln_best_pieces_of(t_count);
    g.p_last = aln_best_pieces_of(g.len_last);
    g.pieces = g.rows == 1u ? g.p_first : g.p_first + (g.rows - 2u) * g.p_full + g.p_last;
    return g;
}

// touched row j (0 .. rows - 1) of the chunk: its first pair as an offset into the chunk, its pairs inside the chunk, its first piece
ALN_BEST_HD inline void aln_best_row_segment(const aln_best_chunk &g, uint64_t t_count, uint64_t j, uint64_t *start, uint64_t *len,
                                             uint64_t *piece0, uint64_t *n_pieces)
{
    if (j == 0) { *start = 0; *len = g.len_first; *piece0 = 0; *n_pieces = g.p_first; return; }
    *start = g.len_first + (j - 1u) * t_count;
    *piece0 = g.p_first + (j - 1u) * g.p_full;
    if (j == g.rows - 1u) { *len = g.len_last; *n_pieces = g.p_last; }
    else { *len = t_count; *n_pieces = g.p_full; }
}

// piece p (0 .. pieces - 1) of the chunk: its touched row j, its first pair as an offset into the chunk, its pairs
ALN_BEST_HD inline void aln_best_piece(const aln_best_chunk &g, uint64_t t_count, uint64_t p, uint64_t *j, uint64_t *start, uint64_t *len)
{
    uint64_t row, in_row;
    if (p < g.p_first) { row = 0; in_row = p; }
    else {
        const uint64_t r = p - g.p_first;         // (the last row's pieces start at a multiple of p_full and are at most p_full)
        row = 1u + r / g.p_full;
        in_row = r % g.p_full;
    }
    uint64_t s, l, p0, np;
    aln_best_row_segment(g, t_count, row, &s, &l, &p0, &np);
    const uint64_t a = in_row * ALN_BEST_PIECE;
    *j = row;
    *start = s + a;
    *len = l - a < ALN_BEST_PIECE ? l - a : ALN_BEST_PIECE;
}

// slots kept per row: a row has t_count pairs
ALN_BEST_HD inline uint32_t aln_best_slots(uint32_t k, uint64_t t_count) { return t_count < k ? (uint32_t)t_count : k; }

// ---- fold: entries of the sorted list (keys, ts, n) that come before (key, t)
ALN_BEST_HD inline uint32_t aln_best_count_before(const uint64_t *keys, const uint32_t *ts, uint32_t n, uint64_t key, uint32_t t)
{
    uint32_t c = 0;
    for (uint32_t i = 0; i < n; ++i) c += aln_best_before(keys[i], ts[i], key, t) ? 1u : 0u;
    return c;
}

// the place of entry i of list A in the fold of A and B; the entry is kept iff its place is below cap
ALN_BEST_HD inline uint32_t aln_best_place(uint32_t i, uint64_t key, uint32_t t, const uint64_t *other_keys, const uint32_t *other_ts,
                                           uint32_t n_other)
{
    return i + aln_best_count_before(other_keys, other_ts, n_other, key, t);
}

// the whole fold, one entry at a time (what the merge kernel's lanes do side by side): (a, na) <- first cap of (a, na) U (b, nb);
// out_* hold cap entries and must not alias the inputs.  Returns the new count.
inline uint32_t aln_best_fold(const uint64_t *a_key, const uint32_t *a_t, uint32_t na, const uint64_t *b_key, const uint32_t *b_t, uint32_t nb,
                              uint32_t cap, uint64_t *out_key, uint32_t *out_t)
{
    for (uint32_t i = 0; i < na; ++i) {
        const uint32_t at = aln_best_place(i, a_key[i], a_t[i], b_key, b_t, nb);
        if (at < cap) { out_key[at] = a_key[i]; out_t[at] = a_t[i]; }
    }
    for (uint32_t i = 0; i < nb; ++i) {
        const uint32_t at = aln_best_place(i, b_key[i], b_t[i], a_key, a_t, na);
        if (at < cap) { out_key[at] = b_key[i]; out_t[at] = b_t[i]; }
    }
    return na + nb < cap ? na + nb : cap;
}
