// mdvt_torch_resize.h -- the index and weight arithmetic of torch's CPU resizes that more than one unit computes (mdvt_mvsa.hip:
// k_bilinear_frames; mdvt_megasam.hip: k_tracker_mask, k_tracker_depth, k_tracker_codes): the bilinear source index and weights, the
// two forms of the bilinear sum (include/mdvt_mvsa.h states them and their decree) and the nearest-exact map
// (include/mdvt_megasam.h).  The units are compiled with -ffp-contract=off: every `*`, `+` and `-` below is one IEEE operation, rounded
// before the next.
#pragma once
#include "mdvt_internal.h"

namespace mdvt {
namespace torch_resize {

// torch's bilinear source index and weights of output index x along an axis of n_in values (align_corners=False), unfused
__device__ __forceinline__ void lin_tap(int x, float scale, int n_in, int& i0, int& i1, float& w0, float& w1)
{
    float src = scale * ((float)x + 0.5f) - 0.5f;
    src = src < 0.0f ? 0.0f : src;
    i0 = src >= (float)(n_in - 1) ? n_in - 1 : (int)src;
    i1 = i0 + 1 < n_in - 1 ? i0 + 1 : n_in - 1;
    float lam = src - (float)i0;
    lam = lam < 0.0f ? 0.0f : lam;
    lam = lam > 1.0f ? 1.0f : lam;
    w0 = 1.0f - lam;
    w1 = lam;
}

// the bilinear sum of the four taps of an output value.  small (uniform): torch's kernel for small outputs, four weights, summed in
// order; otherwise its kernel for the others: the two rows, then the column
__device__ __forceinline__ float lin_mix(bool small, float wy0, float wy1, float wx0, float wx1, float v00, float v01, float v10, float v11)
{
    if (small) return (((wy0 * wx0) * v00 + (wy0 * wx1) * v01) + (wy1 * wx0) * v10) + (wy1 * wx1) * v11;
    const float t0 = wx0 * v00 + wx1 * v01;
    const float t1 = wx0 * v10 + wx1 * v11;
    return wy0 * t0 + wy1 * t1;
}

// torch's CPU nearest-exact map: index x of n_out values -> its source among n_in, scale = fl(float(n_in) / float(n_out))
__device__ __forceinline__ int nex_idx(uint32_t x, float scale, int n_in)
{
    const float f = floorf(((float)x + 0.5f) * scale);
    return f >= (float)(n_in - 1) ? n_in - 1 : (int)f;              // (x and scale are >= 0: so is f)
}

}  // namespace torch_resize
}  // namespace mdvt
