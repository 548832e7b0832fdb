// aln_strand.hip -- device side of aln_seqset_create_stranded (include/aligner_hip_strand.h): the mirrors of a set's n records written
// behind them in the same residue buffer, mirror[j] = map[rec[len - 1 - j]].  aln_strand_rules.h is the rule.
//
// One pass over the residues.  The packed forward residues, `total` bytes from the buffer's start, are cut into chunks of 16 bytes and
// a workgroup of 256 threads takes a tile of 4 KiB, whatever records lie in it: the grid is the same for one record of 10^6 residues
// and for 10^6 records of one.  A thread finds the record of its chunk's first byte by bisection over the offsets the set keeps on the
// device anyway.
//   whole     the chunk lies in one record: one 16-byte load (the buffer's start is aligned and so is every chunk), the 16 bytes
//             through the table in reverse order, one 16-byte store where the mirror's address happens to be aligned, else 16 byte stores
//   ragged    the chunk holds a record's head or tail (or several short records), or is the buffer's last and short: byte by byte,
//             walking on to the next record where one ends; records of no residues are stepped over
// The table is 256 bytes of LDS, one per thread.
//
// Bounds: a load stays below `total`; a store goes to total + off[i] + (len - 1 - j) with j < len, which is below 2 * total, and the
// buffer has 2 * total + 256 bytes.  Every byte of the mirrors is a plain C++ store of exactly one thread.  No atomics, no kernel waits
// for another workgroup.
#include <hip/hip_runtime.h>

#include "aln_launch.h"
#include "aln_strand_rules.h"

static_assert(ALN_STRAND_TILE == 256u * ALN_STRAND_CHUNK, "a tile is one chunk per thread");

__global__ __launch_bounds__(256) void aln_strand_mirror_kernel(uint8_t *seqs, const uint64_t *off, const uint32_t *len, uint64_t n, uint64_t total,
                                                                const uint8_t *map)
{
    __shared__ uint8_t table[256];
    table[threadIdx.x] = map[threadIdx.x];
    __syncthreads();
    const uint64_t first = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * ALN_STRAND_CHUNK;
    if (first >= total || n == 0) return;
    uint64_t i = aln_strand_record_at(off, n, first);
    uint64_t base = off[i], L = len[i];
    if (first + ALN_STRAND_CHUNK <= base + L) {       // whole (base + L <= total)
        const uint4 v = *reinterpret_cast<const uint4 *>(seqs + first);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t r[4];                                // the 16 bytes mapped, in reverse order
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t x = w[3u - k];
            r[k] = (uint32_t)table[x >> 24] | (uint32_t)table[(x >> 16) & 255u] << 8 | (uint32_t)table[(x >> 8) & 255u] << 16 | (uint32_t)table[x & 255u] << 24;
        }
        // the chunk's last byte is the lowest of its mirrors
        uint8_t *dst = seqs + aln_strand_mirror_off(total, base) + aln_strand_mirror_pos(L, first + ALN_STRAND_CHUNK - 1u - base);
        if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) *reinterpret_cast<uint4 *>(dst) = make_uint4(r[0], r[1], r[2], r[3]);
        else for (uint32_t k = 0; k < ALN_STRAND_CHUNK; ++k) dst[k] = (uint8_t)(r[k >> 2] >> (8u * (k & 3u)));
        return;
    }
    const uint64_t end = first + ALN_STRAND_CHUNK < total ? first + ALN_STRAND_CHUNK : total;
    for (uint64_t p = first; p < end; ++p) {          // ragged
        while (p >= base + L && i + 1u < n) { ++i; base = off[i]; L = len[i]; }
        if (p < base || p >= base + L) return;        // (not of a packed set: nothing is written for it)
        seqs[aln_strand_mirror_off(total, base) + aln_strand_mirror_pos(L, p - base)] = table[seqs[p]];
    }
}

// seqs: 2 * total + 256 bytes, the first `total` of them the n records packed in order; off, len: theirs; map: 256 bytes
extern "C" void aln_strand_launch_mirror(uint8_t *seqs, const uint64_t *off, const uint32_t *len, uint64_t n, uint64_t total, const uint8_t *map,
                                         hipStream_t s)
{
    if (n == 0 || total == 0) return;
    hipLaunchKernelGGL(aln_strand_mirror_kernel, dim3((uint32_t)aln_strand_tiles(total)), dim3(256), 0, s, seqs, off, len, n, total, map);
}
