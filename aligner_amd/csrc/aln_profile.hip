// aln_profile.hip -- device side of aln_seqset_held_profiles (include/aligner_hip_profile.h): the columns of the held hits' aligned
// strings counted into the profiles of their families' centres, where the strings lie.  aln_profile_rules.h is the rule; this file is
// its wave64 form.
//
//   slots     one thread per centre: slot_of[centers[i]] = i (the table was filled with ALN_CLUSTER_NONE on the stream before) and
//             record i gets its centre; the counts of the records were zeroed on the stream before
//   count     one wave per held hit, ALN_PROFILE_WAVES hits per workgroup, as aln_report_kernel.  Every lane of the wave reads the
//             hit's summary, endpoints and labels and comes to the same decision (aln_profile_decide); a hit that does not contribute
//             adds one to its counter, from lane 0, and the wave leaves.  Lane l takes columns l, l + 64, ... of both strings: byte
//             loads at consecutive addresses.  The centre position of a column is start + the centre's non-blanks in front of it: a
//             64-bit ballot of "centre non-blank", a popcount of the lanes below, and a base carried from round to round.  One
//             atomicAdd of 1 per counted column goes into the profile, which was zeroed on the stream before.  matched, deleted and
//             overflow are folded across the wave by cross-lane moves at distances 32 .. 1, then lane 0 adds them once
//
// Bounds: a column index stays below aln_len clipped to N + M + 2, the room of one string in the held store; a position is compared
// with len[centre] in 64 bits before it indexes; slot_of is indexed with a sequence number below n_seqs only (never with a label), and
// a slot is compared with n_centers before it indexes.  Atomics: integer adds only, where the result does not depend on their order.
// No barrier, no kernel that waits for another workgroup.  Every other store is a plain C++ store of a thread.
#include <hip/hip_runtime.h>

#include "aln_device.h"
#include "aln_launch.h"
#include "aln_profile_rules.h"

#define ALN_PROFILE_WAVES 4u
#define ALN_PROFILE_THREADS 256u

__global__ __launch_bounds__(256) void aln_profile_slots_kernel(const uint32_t *centers, uint32_t n_centers, uint32_t n_seqs, uint32_t *slot_of,
                                                                aln_profile_record *rec)
{
    const uint64_t i = (uint64_t)blockIdx.x * ALN_PROFILE_THREADS + threadIdx.x;
    if (i >= n_centers) return;
    const uint32_t c = centers[i];
    rec[i].center = c;
    if (c < n_seqs) slot_of[c] = (uint32_t)i;         // (checked on the host; never written beyond the table)
}

__global__ __launch_bounds__(64 * ALN_PROFILE_WAVES) void aln_profile_kernel(ProfileArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t h = (uint64_t)blockIdx.x * ALN_PROFILE_WAVES + (threadIdx.x >> 6);
    if (h >= a.n_held) return;
    // (everything up to the loop is the same for every lane of the wave)
    const aln_pair_result r = a.res[h];
    if (r.status != ALN_OK) return;
    const HeldEntry d = a.held[h];
    if (a.rep && !aln_report_keep(a.rep[h], a.filter, d.N, d.M)) return;
    const uint32_t q = a.hit_q[h], t = a.hit_t[h];
    if (q >= a.n_seqs || t >= a.n_seqs) return;       // checked on the host; never indexed
    uint32_t c = 0, c_is_q = 0, slot = ALN_CLUSTER_NONE;
    uint32_t kind = aln_profile_decide(q, t, a.label[q], a.label[t], &c, &c_is_q);
    if (kind == ALN_PROFILE_SKIP) return;
    if (kind == ALN_PROFILE_COUNTS) {
        slot = c < a.n_seqs ? a.slot_of[c] : ALN_CLUSTER_NONE;        // (c is q or t)
        if (slot >= a.n_centers) kind = ALN_PROFILE_UNLISTED;
    }
    if (kind != ALN_PROFILE_COUNTS) {
        if (lane == 0) atomicAdd(&a.misc[kind], 1ull);
        return;
    }
    const uint32_t cap = d.N + d.M + 2u;
    const uint32_t len = r.aln_len < cap ? r.aln_len : cap;
    const uint32_t n = aln_report_columns(len, a.flags), seed = aln_profile_seed_column(len, a.flags);
    const uint8_t *__restrict__ qs = a.tb + d.tb_off;
    const uint8_t *__restrict__ ts = qs + cap;
    const uint8_t *__restrict__ cs = c_is_q ? qs : ts;
    const uint8_t *__restrict__ ms = c_is_q ? ts : qs;
    const uint32_t start = c_is_q ? r.start_x : r.start_y;
    const uint32_t len_c = a.len[c];
    uint32_t *prof = a.out + a.off[slot];
    uint32_t base = 0, matched = 0, deleted = 0, over = 0;
    for (uint64_t j0 = 0; j0 < n; j0 += 64u) {        // (every lane runs every round: the ballot is the whole wave's)
        const uint64_t j = j0 + lane;
        const bool in = j < n;
        const uint32_t cc = in ? cs[j] : a.blank, mc = in ? ms[j] : a.blank;
        const bool residue = in && cc != a.blank;
        const unsigned long long mask = __ballot(residue);
        if (residue) {
            const uint32_t before = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            const uint64_t pos = aln_profile_position(start, before, (uint32_t)j == seed);
            if (pos < len_c) {
                const uint32_t row = aln_profile_row(mc, a.blank, a.n_codes);
                atomicAdd(&prof[(uint64_t)row * len_c + pos], 1u);
                matched += row < a.n_codes ? 1u : 0u;
                deleted += row == a.n_codes ? 1u : 0u;
            } else {
                over += 1u;
            }
        }
        base += (uint32_t)__popcll(mask);
    }
    for (uint32_t w = 32u; w >= 1u; w >>= 1) {
        matched += __shfl_down(matched, w, 64);
        deleted += __shfl_down(deleted, w, 64);
        over += __shfl_down(over, w, 64);
    }
    if (lane == 0) {
        aln_profile_record *rec = a.rec + slot;
        atomicAdd(&rec->hits, 1u);
        if (matched) atomicAdd(&rec->matched, matched);
        if (deleted) atomicAdd(&rec->deleted, deleted);
        atomicAdd(&a.misc[ALN_PROFILE_COUNTS], 1ull);
        if (over) atomicAdd(&a.misc[ALN_PROFILE_MISC_OVERFLOW], (unsigned long long)over);
    }
}

extern "C" int aln_warm_profile(void)
{
    hipFuncAttributes attr;
    return (int)hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&aln_profile_kernel));
}

// slot_of: n_seqs words, filled with ALN_CLUSTER_NONE before; rec: n_centers records, zeroed before
extern "C" void aln_profile_launch_slots(const uint32_t *centers, uint32_t n_centers, uint32_t n_seqs, uint32_t *slot_of, aln_profile_record *rec,
                                         hipStream_t s)
{
    if (n_centers) hipLaunchKernelGGL(aln_profile_slots_kernel, dim3(blocks_of(n_centers, ALN_PROFILE_THREADS)), dim3(ALN_PROFILE_THREADS), 0, s, centers,
                                      n_centers, n_seqs, slot_of, rec);
}

// out, rec's counts and misc (ALN_PROFILE_MISC_WORDS 64-bit words) zeroed before
extern "C" void aln_profile_launch(const ProfileArgs *a, hipStream_t s)
{
    if (a->n_held)                                    // (without centres too: the summary's counters are the kernel's)
        hipLaunchKernelGGL(aln_profile_kernel, dim3(blocks_of(a->n_held, ALN_PROFILE_WAVES)), dim3(64 * ALN_PROFILE_WAVES), 0, s, *a);
}
