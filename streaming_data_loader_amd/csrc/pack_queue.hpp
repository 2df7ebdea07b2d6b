// pack_queue.hpp -- host bookkeeping of the packed rows' batch queue (sdl_config.pack = 1): where
// the G rows a call emitted land in the working batch and the fresh batches behind it.  Plain
// host code, no HIP: tests/pack_queue_check.cpp runs it under the host sanitizers.
#pragma once

#include <cstdint>
#include <vector>

namespace sdl {

// Rows [g0, g0 + n) of the call go to rows [dst, dst + n) of batch `batch`: 0 is the working
// batch (it holds `fill` rows already), k > 0 the k-th fresh batch after it.
struct PackSeg {
    uint32_t batch, dst, g0, n;
};

struct PackPlan {
    std::vector<PackSeg> segs;  // in row order; every segment lies inside one batch
    uint32_t completed = 0;     // batches 0 .. completed - 1 are full afterwards, in order
    uint32_t fill = 0;          // rows in batch `completed`, the new working batch (< B)
};

// fill < B rows wait in the working batch of B rows; G more arrive.
inline PackPlan pack_queue_plan(uint32_t fill, uint32_t B, uint64_t G) {
    PackPlan p;
    if (B == 0 || fill >= B) return p;  // (not a state the queue is ever in)
    uint64_t g = 0;
    uint32_t batch = 0;
    while (g < G) {
        const uint64_t room = (uint64_t)B - fill;
        const uint32_t n = (uint32_t)(G - g < room ? G - g : room);
        p.segs.push_back(PackSeg{batch, fill, (uint32_t)g, n});
        g += n;
        fill += n;
        if (fill == B) {
            ++batch;
            fill = 0;
        }
    }
    p.completed = batch;
    p.fill = fill;
    return p;
}

}  // namespace sdl
