// mdvt_depth_code.h -- the tail of depth_frames_helper.save_depth_video as device code: NumPy's clip, cv2.resize(INTER_LINEAR)'s tables
// on float32 and the 16-bit RGB depth code with its packed stores.  What mdvt_metric_align.hip (k_metric_codes) and mdvt_depth_sink.hip
// (k_depth_sink) share; include/mdvt_metric_align.h states the arithmetic.  Both units are compiled with -ffp-contract=off: every `*`
// and `+` below is one IEEE operation, rounded before the next.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdvt {
namespace depth_code {

// NumPy's clip(d, 0, hi): a NaN stays, and so does -0
__device__ __forceinline__ float clip_np(float d, float hi)
{
    const float lo = d < 0.0f ? 0.0f : d;
    return lo > hi ? hi : lo;
}

// source index and weight of output index d along an axis of n_in source values: cv2's INTER_LINEAR tables, restated
__device__ __forceinline__ void tap(int d, double ratio, int n_in, int& s0, int& s1, float& w0, float& w1)
{
    float f = (float)(((double)d + 0.5) * ratio - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.0f; }
    if (s >= n_in - 1) { s = n_in - 1; f = 0.0f; }
    s0 = s;
    s1 = s + 1 < n_in - 1 ? s + 1 : n_in - 1;
    w0 = 1.0f - f;
    w1 = f;
}

// the three code bytes of a clipped depth c as the low 24 bits of a word, first byte lowest: u = uint32(trunc(multi * double(c))),
// R = G = byte 3 of u, B = byte 2; bgr: B, G, R.  A NaN gives 0.
__device__ __forceinline__ uint32_t pixel(float c, double multi, int bgr)
{
    const double e = multi * (double)c;
    const uint32_t code = (e >= 0.0 && e < 4294967296.0) ? (uint32_t)e : 0u;     // NaN -> 0
    const uint32_t hi = code >> 24, lo = (code >> 16) & 0xFFu;
    return bgr ? (lo | (hi << 8) | (hi << 16)) : (hi | (hi << 8) | (lo << 16));
}

// the first nv (1 .. 4) of four pixels to q: 12 bytes as three dword stores where vec says q is a multiple of 4, byte by byte otherwise
__device__ __forceinline__ void store_pixels(uint8_t* q, const uint32_t (&px)[4], int nv, bool vec)
{
    if (vec && nv == 4) {
        uint32_t* w = reinterpret_cast<uint32_t*>(q);
        w[0] = px[0] | (px[1] << 24);
        w[1] = (px[1] >> 8) | (px[2] << 16);
        w[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < nv) {
                q[3 * k] = (uint8_t)px[k]; q[3 * k + 1] = (uint8_t)(px[k] >> 8); q[3 * k + 2] = (uint8_t)(px[k] >> 16);
            }
        }
    }
}

// the first nv of four float32 values to z: one 16-byte store where vec says z is a multiple of 16
__device__ __forceinline__ void store_plane(float* z, const float (&d)[4], int nv, bool vec)
{
    if (vec && nv == 4) {
        *reinterpret_cast<float4*>(z) = make_float4(d[0], d[1], d[2], d[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nv) z[k] = d[k];
    }
}

}  // namespace depth_code
}  // namespace mdvt
