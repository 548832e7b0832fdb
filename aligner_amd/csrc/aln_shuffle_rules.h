// aln_shuffle_rules.h -- the shuffled copies of a target that aln_shuffle_scores / aln_shuffle_targets align (the device
// counterpart of shuffle_and_randomize_sequence, statistics/mod.rs:309-320): plain arithmetic, no HIP, so that the host plan, the
// shuffle kernel (aln_shuffle.hip) and a CPU test driver compute the same copies.
//
//   stream    copy s of pair i has a SplitMix64 state of its own:
//               seed ^ ((pair_base + i) * 0xD1B54A32D192ED03) ^ ((s + 1) * 0xABC98388FB8FAC03)       (uint64, wrapping)
//             so a copy depends on (seed, pair_base + i, s) only -- not on chunking, launch geometry or how a job's pairs are
//             split across calls.
//   bounded   bounded(n), 1 <= n < 2^32: Lemire's multiply-shift with rejection on the upper 32 bits of next().
//   trim      the first draw, bounded(max_trim + 1): the copy is target[0 .. L - trim) (statistics/mod.rs:312-314).
//   shuffle   Fisher-Yates in the order of rand 0.8's SliceRandom::shuffle: for k = L' - 1 down to 1, swap(a[k], a[bounded(k + 1)]).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define ALN_HD __host__ __device__
#else
#define ALN_HD
#endif

// the state of copy s of pair `pair` (= pair_base + i)
ALN_HD inline uint64_t aln_shuffle_state(uint64_t seed, uint64_t pair, uint64_t s)
{
    return seed ^ (pair * 0xD1B54A32D192ED03ull) ^ ((s + 1) * 0xABC98388FB8FAC03ull);
}

// SplitMix64
ALN_HD inline uint64_t aln_shuffle_next(uint64_t &state)
{
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// uniform in [0, n), 1 <= n < 2^32
ALN_HD inline uint32_t aln_shuffle_bounded(uint64_t &state, uint32_t n)
{
    uint64_t m = (aln_shuffle_next(state) >> 32) * (uint64_t)n;
    if ((uint32_t)m < n) {
        const uint32_t t = (uint32_t)(0u - n) % n;
        while ((uint32_t)m < t) m = (aln_shuffle_next(state) >> 32) * (uint64_t)n;
    }
    return (uint32_t)(m >> 32);
}

// tail residues copy s drops: the first draw of its stream (advances the state past it)
ALN_HD inline uint32_t aln_shuffle_trim(uint64_t &state, uint32_t max_trim)
{
    return aln_shuffle_bounded(state, max_trim + 1u);
}

// the trim of copy s of pair `pair` alone (the host plan and the descriptor expansion need the lengths, not the copies)
ALN_HD inline uint32_t aln_shuffle_trim_of(uint64_t seed, uint64_t pair, uint64_t s, uint32_t max_trim)
{
    uint64_t state = aln_shuffle_state(seed, pair, s);
    return aln_shuffle_trim(state, max_trim);
}

// Fisher-Yates over a[0 .. len), continuing the stream after the trim draw
template <class P>
ALN_HD inline void aln_shuffle_permute(uint64_t &state, P a, uint32_t len)
{
    for (uint32_t k = len; k-- > 1;) {
        const uint32_t j = aln_shuffle_bounded(state, k + 1u);
        const uint8_t v = a[k];
        a[k] = a[j];
        a[j] = v;
    }
}
