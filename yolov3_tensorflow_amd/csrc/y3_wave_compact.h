// Compaction in order inside one 64-wide wavefront (y3_mosaic.hip, y3_affine.hip: one wavefront walks an image's candidate
// boxes in chunks of 64 and writes the kept ones behind those of the chunks before).
#pragma once

namespace y3wc {

constexpr int kWave = 64;

static_assert(sizeof(unsigned long long) * 8 == kWave, "the ballot mask holds one bit per lane of a 64-wide wavefront");

// Called by all 64 lanes together.  kept: how many the chunks before kept (uniform over the wavefront), moved on by this
// chunk's number.  Returns the slot of this lane's candidate - meaningful where keep holds - in ascending lane order.
__device__ __forceinline__ int compact_slot(bool keep, int lane, int& kept) {
    const unsigned long long mask = __ballot(keep);
    const int at = kept + __popcll(mask & ((1ull << lane) - 1ull));
    kept += __popcll(mask);
    return at;
}

}  // namespace y3wc
