// aln_plan_rules.h -- decisions of the batch plan (aln_host.hip) that are plain arithmetic on the plan's figures: no HIP, so
// that a test can compile them on a machine without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

// Which build of the fast batch kernel a chunk that could share strips runs: with the cooperative machinery (COOP = true) or
// without it (the lean build).
//
// With more than two pairs per resident wave nobody opens a first pass (FillArgs::coop_tail); what can still be shared are the
// re-fills opened while fewer than two pairs per kernel wave are left in the queue (fast_work: taken + 2 x waves >= pairs) --
// re-fills of the pairs whose first pass ends then.  In an LPT queue (longest first) those are
//   * the pairs of the queue's tail, its last 2 x waves positions: the first of them is the longest, and
//   * pairs taken early whose first pass lasts into the tail: only a pair that costs a good part of a wave's share can.
// So the lean build is chosen when there are many pairs per resident wave, the tail's longest pair is a small fraction of a
// wave's share (a re-fill of it, alone on one wave, delays little), and the queue's longest pair is at most a quarter of a
// wave's share (its first pass and a re-fill are through before the tail begins, so no build could have shared that re-fill).
// Sharing there shortens next to nothing, while the machinery is paid for in every step of every pair (C5, 100 000 pairs:
// 14.26 against 14.08 VALU instructions per cell, 46.4 against 43.5 GB per launch, fill 45.4 against 43.9 ms).
//
// Costs are in pair_cost units (aln_host.hip: the time one wave needs for the pair); cost_at(j) = cost of queue position j, the
// queue in LPT order.  grid: the kernel's workgroups of four waves; cus: the device's CUs (three workgroups each are resident).
// setting: ALN_COOP_LEAN (< 0 unset, 0 never lean, > 0 always lean).
static constexpr uint64_t ALN_LEAN_MIN_PAIRS_PER_WAVE = 16;   // at least this many pairs per resident wave
static constexpr double ALN_LEAN_TAIL_FRACTION = 1.0 / 64.0;  // the tail's longest pair: at most this share of a wave's work
static constexpr double ALN_LEAN_MAX_FRACTION = 1.0 / 4.0;    // the queue's longest pair: at most this share

struct AlnLeanPlan {
    uint64_t waves, resident, tail;    // kernel waves, resident waves, queue position of the tail's first (longest) pair
    double share;                      // a resident wave's share of the batch (pair_cost units)
    bool lean;
};

template <class CostAt>
inline AlnLeanPlan aln_coop_lean_plan(uint64_t n_pairs, uint32_t grid, uint32_t cus, double total_cost, CostAt cost_at, int setting)
{
    AlnLeanPlan p;
    p.waves = (uint64_t)grid * 4u;
    p.resident = (uint64_t)cus * 3u * 4u;
    p.tail = n_pairs > 2 * p.waves ? n_pairs - 2 * p.waves : 0;
    const uint64_t w = p.waves < p.resident ? p.waves : p.resident;
    p.share = w ? total_cost / (double)w : 0.0;
    if (setting >= 0) p.lean = setting > 0;
    else if (w == 0 || n_pairs == 0 || n_pairs < ALN_LEAN_MIN_PAIRS_PER_WAVE * w) p.lean = false;
    else p.lean = (double)cost_at((size_t)p.tail) <= ALN_LEAN_TAIL_FRACTION * p.share &&
                  (double)cost_at((size_t)0) <= ALN_LEAN_MAX_FRACTION * p.share;
    return p;
}
