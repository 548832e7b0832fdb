// aln_loop_rules.h -- the decision of one iteration of the heuristic loop (heuristic/mod.rs:64-75) for one pair, as the library takes
// it on the device (aln_pairset_loop_step, aln_loop.hip): plain C++, no HIP, so that the kernel and a CPU test driver decide alike.
//
//   status != ALN_OK          the pair failed: finished, cause ALN_LOOP_CAUSE_FAILED (its status is in its summary)
//   f > best                  a plain IEEE compare (false for a NaN on either side, and for +0.0 against -0.0): the pair improved;
//                             best = f, and its matrix is re-estimated.  If the transform then finds no root, the pair is finished,
//                             cause ALN_LOOP_CAUSE_NO_ROOT; otherwise it goes on
//   otherwise                 finished, cause ALN_LOOP_CAUSE_DONE: the result of HeuristicAligner
#pragma once
#include <stdint.h>

#include "../../include/aligner_hip.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define ALN_LOOP_HD __host__ __device__
#else
#define ALN_LOOP_HD
#endif

// the cause of a finished pair (aln_pairset_loop_step's `cause`)
#define ALN_LOOP_CAUSE_DONE 0u
#define ALN_LOOP_CAUSE_FAILED 1u
#define ALN_LOOP_CAUSE_NO_ROOT 2u
// the classes of an entry inside a step: a cause, or one of these
#define ALN_LOOP_IMPROVED 3u      // f > best: waits for its transform
#define ALN_LOOP_GOING 4u         // improved and re-estimated: in the next step's going list

// the class of an entry after its run, before any transform: a cause (DONE, FAILED) or ALN_LOOP_IMPROVED
ALN_LOOP_HD inline uint32_t aln_loop_classify(int32_t status, double f, double best)
{
    if (status != ALN_OK) return ALN_LOOP_CAUSE_FAILED;
    return f > best ? ALN_LOOP_IMPROVED : ALN_LOOP_CAUSE_DONE;
}

// the class of an improved entry once its transform has answered
ALN_LOOP_HD inline uint32_t aln_loop_after_transform(int32_t transform_status)
{
    return transform_status == 0 ? ALN_LOOP_GOING : ALN_LOOP_CAUSE_NO_ROOT;
}

// which list of a step an entry's class puts it on
ALN_LOOP_HD inline bool aln_loop_is_finished(uint32_t cls) { return cls <= ALN_LOOP_CAUSE_NO_ROOT; }
