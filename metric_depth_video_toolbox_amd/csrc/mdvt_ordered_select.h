// mdvt_ordered_select.h -- the two steps that every "mean of the selected values, in row-major order" shares (mdvt_convergence.hip:
// k_conv_scan, k_conv_mean; mdvt_depth_engines.hip: k_focal_scan, k_focal_mean).  A list's values are selected per unit of 2048, the
// unit counts are scanned into the units' places (unit_scan), the selected values are compacted and summed per chunk of 8192 in
// NumPy's order (mdvt_pairwise.h), and the chunk sums make the mean (ordered_mean).  How a unit selects, compacts and reduces is
// each unit's own.  Both functions are called by all 64 lanes of a workgroup of one wave.
#pragma once

#include "mdvt_pairwise.h"

namespace mdvt {
namespace ordered_select {

// off[i] = cnt[0] + .. + cnt[i - 1] for the nunits units of a list, *total_out = the list's count: 64 units a step, with a carry
__device__ __forceinline__ void unit_scan(const uint32_t* cnt, uint32_t* off, uint32_t nunits, uint32_t* total_out)
{
    const int lane = (int)threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nunits; base += 64u) {
        const uint32_t i = base + (uint32_t)lane;
        const uint32_t v = i < nunits ? cnt[i] : 0u;
        uint32_t s = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(s, d);
            if (lane >= d) s += t;
        }
        if (i < nunits) off[i] = carry + s - v;
        carry += __shfl(s, 63);
    }
    if (lane == 0) *total_out = carry;
}

// the mean of a list of `total` values from its chunk sums: the sums added one after the other (64 loaded a step, then taken lane by
// lane), one division by float(total); `empty` where the list is
__device__ __forceinline__ float ordered_mean(const float* sums, uint32_t total, float empty)
{
    const int lane = (int)threadIdx.x;
    const uint32_t nch = (total + (uint32_t)pairwise::kChunk - 1u) / (uint32_t)pairwise::kChunk;
    float acc = 0.f;
    for (uint32_t base = 0; base < nch; base += 64u) {
        const float s = base + (uint32_t)lane < nch ? sums[base + (uint32_t)lane] : 0.f;
        const int m = (int)(nch - base < 64u ? nch - base : 64u);
        for (int j = 0; j < m; ++j) acc += __shfl(s, j);
    }
    return total ? acc / (float)total : empty;
}

}  // namespace ordered_select
}  // namespace mdvt
