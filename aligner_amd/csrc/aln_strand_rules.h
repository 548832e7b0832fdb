// aln_strand_rules.h -- a sequence set on both strands (aln_seqset_create_stranded, aln_seqset_held_strand_cigar_plan / _fill,
// include/aligner_hip_strand.h): where the mirrors lie, which strand a hit is on, its coordinates on the original records and where a
// word of its CIGAR goes.  Integer arithmetic only, no HIP, so that the kernels (aln_strand.hip, aln_cigar.hip), the host and a CPU test
// driver decide all of it the same way.
//
//   set        n records become 2n: record n + i is the mirror of record i, mirror[j] = map[rec[len - 1 - j]]; off[n + i] = total +
//              off[i], total the residues of the n records; the residue buffer has 2 * total + 256 bytes.  2n < 2^32
//   hit        (q_seq, t_seq) of the 2n: qm = q_seq >= n, tm = t_seq >= n, q_rec = q_seq mod n, t_rec = t_seq mod n, '-' iff qm != tm
//   record     the plain plan's with (start, end) -> (L - end, L - start) on a mirrored side, L that record's length; a status that
//              is not ALN_OK: the plain plan's all-zero record as it is
//   words      the plain plan's, word r at place n_ops - 1 - r iff tm (clips included: they change places with the rest)
#pragma once
#include <stdint.h>

#include "../../include/aligner_hip_strand.h"
#include "aln_cigar_rules.h"

#define ALN_STRAND_TILE 4096u                     // residues a workgroup of the mirror kernel takes: 256 threads of 16 bytes
#define ALN_STRAND_CHUNK 16u
#define ALN_STRAND_SLACK 256u                     // bytes behind the residues, as aln_seqset_create leaves them

ALN_CIGAR_PIN(strand_size, sizeof(aln_strand_record) == 16);
ALN_CIGAR_PIN(strand_q_rec, __builtin_offsetof(aln_strand_record, q_rec) == 0);
ALN_CIGAR_PIN(strand_t_rec, __builtin_offsetof(aln_strand_record, t_rec) == 4);
ALN_CIGAR_PIN(strand_strand, __builtin_offsetof(aln_strand_record, strand) == 8);
ALN_CIGAR_PIN(strand_q_mirror, __builtin_offsetof(aln_strand_record, q_mirror) == 9);
ALN_CIGAR_PIN(strand_t_mirror, __builtin_offsetof(aln_strand_record, t_mirror) == 10);
ALN_CIGAR_PIN(strand_reserved, __builtin_offsetof(aln_strand_record, reserved) == 11);
ALN_CIGAR_PIN(strand_reserved2, __builtin_offsetof(aln_strand_record, reserved2) == 12);

// ---- the set
ALN_CIGAR_HD inline bool aln_strand_count_ok(uint64_t n) { return n < (1ull << 31); }           // 2n < 2^32
ALN_CIGAR_HD inline uint64_t aln_strand_buffer_bytes(uint64_t total) { return 2ull * total + ALN_STRAND_SLACK; }
ALN_CIGAR_HD inline uint64_t aln_strand_mirror_off(uint64_t total, uint64_t off) { return total + off; }
ALN_CIGAR_HD inline uint64_t aln_strand_tiles(uint64_t total) { return (total + ALN_STRAND_TILE - 1u) / ALN_STRAND_TILE; }
// residue j of a record of len residues is residue len - 1 - j of its mirror (j < len)
ALN_CIGAR_HD inline uint64_t aln_strand_mirror_pos(uint64_t len, uint64_t j) { return len - 1ull - j; }

// the record among n (off ascending, lengths len) that holds residue position p of the packed buffer, p < off[n - 1] + len[n - 1]:
// the last one whose off is at or below p (the records of no residues that share its off come before it)
template <class Off> ALN_CIGAR_HD inline uint64_t aln_strand_record_at(const Off *off, uint64_t n, uint64_t p)
{
    uint64_t lo = 0, hi = n;                          // off[lo] <= p < off[hi] (off[n]: beyond all)
    while (hi - lo > 1u) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if ((uint64_t)off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- a hit
ALN_CIGAR_HD inline aln_strand_record aln_strand_classify(uint32_t q_seq, uint32_t t_seq, uint32_t n)
{
    aln_strand_record s;
    s.q_mirror = q_seq >= n ? 1u : 0u;
    s.t_mirror = t_seq >= n ? 1u : 0u;
    s.q_rec = s.q_mirror ? q_seq - n : q_seq;
    s.t_rec = s.t_mirror ? t_seq - n : t_seq;
    s.strand = s.q_mirror != s.t_mirror ? (uint8_t)'-' : (uint8_t)'+';
    s.reserved = 0; s.reserved2 = 0;
    return s;
}

// (start, end) of a mirror on its original record of len residues (an end beyond len -- not of a set's own strings -- is held at len)
ALN_CIGAR_HD inline void aln_strand_flip(uint32_t len, uint32_t *start, uint32_t *end)
{
    const uint32_t s = *start < len ? *start : len, e = *end < len ? *end : len;
    *start = len - e;
    *end = len - s;
}

// the stranded record of a plain one: N, M the lengths of the hit's query and target
ALN_CIGAR_HD inline aln_cigar_record aln_strand_record_of(aln_cigar_record r, const aln_strand_record &s, uint32_t N, uint32_t M)
{
    if (r.status != ALN_OK) return r;
    if (s.q_mirror) aln_strand_flip(N, &r.q_start, &r.q_end);
    if (s.t_mirror) aln_strand_flip(M, &r.t_start, &r.t_end);
    return r;
}

// where word r of the plain plan's n_ops words goes (r < n_ops)
ALN_CIGAR_HD inline uint64_t aln_strand_word_pos(uint64_t r, uint32_t n_ops, bool reversed) { return reversed ? (uint64_t)n_ops - 1ull - r : r; }
