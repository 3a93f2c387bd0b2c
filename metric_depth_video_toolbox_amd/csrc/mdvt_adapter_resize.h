// mdvt_adapter_resize.h -- THE U8 RESIZE of include/mdvt_infill_adapter.h on the device, shared by the units that resize frames for a
// model (mdvt_infill_adapter.hip, mdvt_infill_engines.hip).  Integer arithmetic apart from the two tap fractions, which are float32
// as the header states them; the including unit is compiled with -ffp-contract=off.
#pragma once

#include "mdvt_device.h"

namespace mdvt {

struct Tap { int s0, s1, w0, w1; };

// cv2's INTER_LINEAR tables for uint8 (11 fractional bits), restated: source indices and integer weights of output index d.
// Columns zero the fraction where the index is clamped; rows keep it and clamp the two rows instead.
__device__ __forceinline__ Tap adapter_tap(int d, double ratio, int n_in, bool column)
{
    float f = (float)(((double)d + 0.5) * ratio - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (column) {
        if (s < 0) { s = 0; f = 0.0f; }
        if (s >= n_in - 1) { s = n_in - 1; f = 0.0f; }
    }
    Tap t;
    t.w0 = (int)rintf((1.0f - f) * 2048.0f);
    t.w1 = (int)rintf(f * 2048.0f);
    t.s0 = min(max(s, 0), n_in - 1);
    t.s1 = min(max(s + 1, 0), n_in - 1);
    return t;
}

// One output pixel (three channels packed as R | G << 8 | B << 16) of the u8 resize; px(sx, sy) gives a source pixel.
template <class Fetch>
__device__ __forceinline__ uint32_t adapter_resize_px(const AdapterResize& r, int dx, int dy, Fetch px)
{
    if (r.mode == 0) return px(dx, dy);
    if (r.mode == 1) {
        const uint32_t a = px(2 * dx, 2 * dy), b = px(2 * dx + 1, 2 * dy), c = px(2 * dx, 2 * dy + 1), d = px(2 * dx + 1, 2 * dy + 1);
        uint32_t o = 0;
#pragma unroll
        for (int k = 0; k < 24; k += 8) o |= ((((a >> k) & 0xFFu) + ((b >> k) & 0xFFu) + ((c >> k) & 0xFFu) + ((d >> k) & 0xFFu) + 2u) >> 2) << k;
        return o;
    }
    const Tap tx = adapter_tap(dx, r.rx, r.in_w, true), ty = adapter_tap(dy, r.ry, r.in_h, false);
    const uint32_t p00 = px(tx.s0, ty.s0), p01 = px(tx.s1, ty.s0), p10 = px(tx.s0, ty.s1), p11 = px(tx.s1, ty.s1);
    uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < 24; k += 8) {
        const int h0 = (int)((p00 >> k) & 0xFFu) * tx.w0 + (int)((p01 >> k) & 0xFFu) * tx.w1;
        const int h1 = (int)((p10 >> k) & 0xFFu) * tx.w0 + (int)((p11 >> k) & 0xFFu) * tx.w1;
        const int v = (((ty.w0 * (h0 >> 4)) >> 16) + ((ty.w1 * (h1 >> 4)) >> 16) + 2) >> 2;
        o |= (uint32_t)min(max(v, 0), 255) << k;                 // (cv2's saturate_cast; the weights of an axis sum to 2048)
    }
    return o;
}

}  // namespace mdvt
