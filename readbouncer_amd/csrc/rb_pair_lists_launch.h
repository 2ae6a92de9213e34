// rb_pair_lists_launch.h -- what rb_pair_lists.hip offers the engine: the pair table's census and builder, and the count kernel's launch.
#pragma once
#include <hip/hip_runtime.h>

#include "rb_device.h"
#include "rb_pair_lists.h"

namespace rb {

// Pair form (rb_pair_lists.hip, ibf_count_pair_lists_kernel; rb_pair_lists.h): both strands of a k-mer from ONE three-line slot, one
// workgroup of rbpair::kPairWaves waves per read.  `count` is the launch the list form would make: the pair form serves what
// list_form_serves serves, and the reads with a base outside ACGT are written by the same three-hash twin, launched behind.
struct PairCountLaunch {
    CountLaunch count;
    const uint32_t *slots;  // the filter's pair table (resident form)
    const uint32_t *tails;  // ... its tail lines, tail_rows of them
    const uint64_t *side;   // ... and its dense rows, side_rows of them (pairs)
    uint32_t tail_rows, side_rows;
};
bool pair_form_serves(const CountLaunch &a);
hipError_t launch_ibf_count_pair_lists(const PairCountLaunch &a, hipStream_t st);
// counters[1] += pairs (x, rc(x)), x among 0, step, 2 step, ... < n_rows, that need a tail or more; counters[2] += those that need dense
// rows; counters[0], counters[3] += those whose row(x) lists more than 64, 128 bins; counters start zeroed
hipError_t launch_pair_census(const IbfDev &f, uint32_t *counters, uint64_t n_rows, uint64_t step, hipStream_t st);
// slots <- the pair table, tails <- the tail lines (at most tail_cap are written), side <- the dense row pairs (at most side_cap rows);
// counters[0] += 2 per dense slot, counters[1] += 1 per tail slot; counters start zeroed
hipError_t launch_pair_table(const IbfDev &f, uint32_t *slots, uint32_t *tails, uint64_t *side, uint32_t *counters, uint64_t n_rows,
                             uint32_t tail_cap, uint32_t side_cap, hipStream_t st);

}  // namespace rb
