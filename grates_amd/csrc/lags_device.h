// Device code that the kernels of lags.hip (auto and cross lags) and lags_long.hip share: the reading of a segment table.
#pragma once

#include "common.h"

namespace shg {

// the table clamped to 0 .. M and made non-decreasing: start = max of the clamped entries 0 .. s, end = max(start, entry s + 1); all
// lanes of the wave call it and get the same values
__device__ inline void segment_range(const int32_t* __restrict__ seg, int s, int M, int lane, int& start, int& end) {
    start = 0;
    for (int i = lane; i <= s; i += 64) start = max(start, min(max(seg[i], 0), M));
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) start = max(start, __shfl_xor(start, mask));
    end = max(start, min(max(seg[s + 1], 0), M));
}

}  // namespace shg
