// aln_layout_rules.h -- the pair descriptor and the size arithmetic of the device layout (direction strips, LDS of every fill route,
// advice rows): plain integer arithmetic, no HIP, so that the kernels, the host plan (aln_plan_rules.h) and a CPU test driver size
// every region the same way.  The layout itself is described at the head of aln_device.h, which includes this file.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define ALN_HD __host__ __device__
#else
#define ALN_HD
#endif

#ifndef ALN_FULL_R
#define ALN_FULL_R 8             // rows per lane in a full strip of the batch kernels
#endif
#define ALN_STRIP_ROWS (64 * ALN_FULL_R)   // rows per full strip

struct PairDesc {
    uint64_t q_off, t_off;   // into seqs
    uint32_t N, M;           // query / target length
    uint64_t dir_off;        // into dirs, multiple of 256
    uint64_t tb_off;         // into tb
    uint64_t tag_off;        // into tags
    uint64_t h_off;          // element offset into the optional H matrix buffer
    int32_t status;          // pre-validation status; != 0 -> kernels skip the pair
    uint32_t layout;         // written by the fill kernel
};
// pre-validation status "nothing to align, and the reference returns Ok": PWMAligner with an empty sequence (pwm/mod.rs:52-108:
// the loops do not run, argmax is (0, 0), the traceback stops at once, f = 0).  The kernels skip the pair and report ALN_OK.
#define ALN_PRE_EMPTY_OK (-1)

// aln_pairset_run: four waves' matrices of at most ALN_PAIRSET_MAX_ENTRIES doubles each
ALN_HD inline uint32_t aln_pairset_lds_bytes(uint32_t rows, uint32_t cols) { return 4u * 8u * ((rows * cols + 1u) & ~1u); }

// cooperative passes of the fast batch kernel (CoopRec, aln_device.h): the most strips a shared pass may have, the control words in
// front of the claim words, and the bytes of one record (aln_device.h asserts that this is sizeof(CoopRec))
#define ALN_COOP_MAX_NS 64u
#define ALN_COOP_CTL_WORDS 256u   // (128 ..: diagnostics)
#define ALN_COOP_REC_BYTES (8u + ALN_COOP_MAX_NS * 5u * 8u)

// strip 0 of a hazard pair checkpoints its lane state at steps max(16, one quad), then doubling, up to 1024 (r02: 512 -- enough for
// BLOSUM62 11 / 2, whose bottom-row zeros sit next to the left border; under costlier gaps -- BLOSUM62 x 2 with 46 / 9, the integer
// form of the dyadic scheme x 0.5 with 11.5 / 2.25 -- 41 % of C5's pairs flipped an advice bit beyond column 512 and were re-filled)
#define ALN_CK_SLOTS 7
#define ALN_CASCADE_ROWS 3u

#define ALN_WG_RING 256u      // entries of a hand-off ring (a strip's bottom row, by column & 255)
ALN_HD inline uint32_t aln_wg_lds_bytes(uint32_t rows, uint32_t cols, uint32_t sc_size, uint32_t ns, uint32_t N)
{
    return ((rows * cols * sc_size + 15u) & ~15u) + ns * ALN_WG_RING * sc_size + 3u * ((N + 66u + 15u) & ~15u) + 64u * 4u + ns * 32u +
           (N <= 2048u ? (((N + 66u) * sc_size + 15u) & ~15u) : 0u);      // row 1 of the pass: in LDS for short queries, else in the scratch
}
// LDS of the fast batch kernels (aln_fill_fast_kernel): [S][four waves' profiles][four waves' feed rings: query ring, boundary ring];
// feed_bytes = 0 gives the offset of the rings.  PWM scoring (prof_stride == 0) has neither profiles nor rings.  C5 (24 x 24,
// 12 KiB profiles): 51 456 + 1 856 = 53 312 bytes; three workgroups per CU fit up to 53 760 each (42 of the CU's 128 allocation
// units of 1 280 bytes).
#define ALN_QRING_BYTES 192u  // per wave: 128 query codes + the first 64 once more (aln_fast.h)
#define ALN_BRING_BYTES 272u  // per wave: ints 1 .. 64 hold the 64 columns of the row above that the strip takes next
#define ALN_FEED_BYTES (ALN_QRING_BYTES + ALN_BRING_BYTES)
ALN_HD inline uint32_t aln_fast_lds_bytes(uint32_t rows, uint32_t cols, uint32_t prof_stride, uint32_t feed_bytes)
{
    const uint32_t s_bytes = (rows * cols * 4u + 15u) & ~15u;
    return prof_stride == 0u ? s_bytes : s_bytes + 4u * prof_stride + 4u * feed_bytes;
}

// single-pair kernel: entries of the LDS hand-off ring between two waves of a workgroup (aln_fast.h)
#define ALN_RING 4096u
// LDS bytes of the single-pair fill kernel for W waves per workgroup (rings + S + query offsets + per-wave profile and boundary ring)
ALN_HD inline uint32_t aln_single_lds_bytes(uint32_t rows, uint32_t cols, uint32_t R, uint32_t N, uint32_t W)
{
    const uint32_t s_bytes = (rows * cols * 4u + 15u) & ~15u, prof_bytes = (cols * 64u * R + 15u) & ~15u;
    const uint32_t qo_bytes = ((N + 192u) * 2u + 15u) & ~15u;
    return (W - 1u) * 4u * ALN_RING + s_bytes + qo_bytes + W * (prof_bytes + 512u) + 768u;      // + scratch words (aligned up)
}
// bytes of the single-pair kernel's advice array and of its bottom-row record (one direction dword per block of the last
// strip, at most (N + 63) / 2 + 4 blocks at R = 8), equal sizes, 256-aligned
ALN_HD inline uint64_t single_advice_bytes(uint64_t N)
{
    const uint64_t a = N + 128, z = 4 * ((N + 63) / 2 + 8);
    return ((a > z ? a : z) + 255) & ~255ull;
}

ALN_HD constexpr inline uint32_t aln_spb(uint32_t R) { return R >= 5 ? 2u : R >= 3 ? 4u : 16u / R; }
// rows handled per lane in the strip that starts `rem` rows before the end of the target: the smallest R with 64 R >= rem.
// (A strip costs R cells of issue per step whatever its number of busy lanes; with R in {1,2,4,8} only, the last strips of C5
// were rounded up by 8 % of the batch's work; every R in 1..8 leaves 3 %.)  Steps per direction word: aln_spb(R), the
// largest power of two <= 16 / R (16, 8, 4, 4, 2, 2, 2, 2): the step arithmetic of fill and walk stays shifts and masks, and
// the words of R = 3, 5, 6, 7 simply leave their low bits unused (12, 10, 12, 14 of 16 cell slots filled).
ALN_HD inline int aln_pick_r(uint32_t rem)
{
    const int r = (int)((rem + 63u) / 64u);
    return r > ALN_FULL_R ? ALN_FULL_R : (r < 1 ? 1 : r);
}
ALN_HD inline uint32_t aln_num_strips(uint32_t M) { return (M + ALN_STRIP_ROWS - 1) / ALN_STRIP_ROWS; }
// blocks (of SPB steps) a strip of `nsteps` steps stores, padded to whole quads
ALN_HD inline uint32_t aln_strip_blocks(uint32_t nsteps, uint32_t spb) { return (((nsteps + spb - 1) / spb) + 3u) & ~3u; }
// bytes of one full (R = 8) strip region: steps N+63, 2 steps per block, 256 B per block
ALN_HD inline uint64_t aln_strip_bytes(uint32_t N) { return (uint64_t)aln_strip_blocks(N + 63, aln_spb(ALN_FULL_R)) * 256u; }
// bytes of one strip of the uniform-R layout (single-pair kernel)
ALN_HD inline uint64_t aln_uniform_strip_bytes(uint32_t N, uint32_t R) { return (uint64_t)aln_strip_blocks(N + 63, aln_spb(R)) * 256u; }
ALN_HD inline uint64_t aln_rowmajor_bytes(uint32_t N, uint32_t M)
{
    return (uint64_t)(M + 1) * ((N + 4) / 4);
}
// rows per lane of a cooperative re-fill's uniform strips: at most eight strips up to 2048 rows; 0 = keep the skewed layout
ALN_HD inline uint32_t aln_coop_uniform_r(uint32_t M)
{
    if (M <= 64u || M > 2048u) return 0u;
    return M <= 512u ? 1u : M <= 1024u ? 2u : 4u;
}
ALN_HD inline uint64_t aln_dir_bytes(uint32_t N, uint32_t M)
{
    uint64_t a = (uint64_t)aln_num_strips(M) * aln_strip_bytes(N);
    uint64_t b = aln_rowmajor_bytes(N, M);
    uint64_t m = a > b ? a : b;
    const uint32_t R = aln_coop_uniform_r(M);
    if (R) {
        const uint64_t c = (uint64_t)((M + 64u * R - 1u) / (64u * R)) * aln_uniform_strip_bytes(N, R);
        m = c > m ? c : m;
    }
    return (m + 255) & ~(uint64_t)255;
}
