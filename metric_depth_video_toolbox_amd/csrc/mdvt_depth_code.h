// mdvt_depth_code.h -- what the steps that take a frame four output pixels per thread share (mdvt_metric_align.hip: k_metric_codes;
// mdvt_depth_sink.hip: k_depth_sink, k_depth_sink_up; mdvt_depth_engines.hip: k_model_frames, k_depth_prompt; mdvt_video_mask.hip:
// k_mask_planar).  The frame: a thread's four pixels (Quad, quad_of).  The gather: the source values of a quad, at the same size or
// through cv2.resize(INTER_LINEAR)'s tables on float32 (tap, quad_gather over a source policy, quad_values for float32 planes).
// The tail of depth_frames_helper.save_depth_video: NumPy's clip, the 16-bit RGB depth code and the packed stores (codes_out).
// include/mdvt_metric_align.h states the arithmetic.  The units are compiled with -ffp-contract=off: every `*` and `+` below is one
// IEEE operation, rounded before the next.
#pragma once
#include "mdvt_internal.h"

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

// Four output pixels of a row: columns x0 .. x0 + nv - 1 (nv 1 .. 4) of row `row` of frame f.
struct Quad { uint32_t row; int x0, nv; size_t f; };

// the quad of a thread of a launch of 256-thread workgroups over `groups` = gw * rows quads, a frame per blockIdx.y from frame0 on;
// false for the threads beyond the image
__device__ __forceinline__ bool quad_of(uint32_t groups, uint32_t gw, int out_w, int frame0, Quad& q)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= groups) return false;
    q.row = t / gw;
    q.x0 = (int)(4u * (t - q.row * gw));
    q.nv = out_w - q.x0 < 4 ? out_w - q.x0 : 4;
    q.f = (size_t)frame0 + blockIdx.y;
    return true;
}

// The source values of a quad into out (the values beyond nv stay as they are).  src: the frame; vec: four values from a multiple of 4
// on are one aligned load.  Same size: the quad's own four values.  Resized: every pixel's four taps, filtered horizontally, then
// vertically.  Source: kBytes per stored value, at(p, x) gives value x from p on as float32, four(p, d) values 0 .. 3 in one load.
template <class Source>
__device__ __forceinline__ void quad_gather(float (&out)[4], const uint8_t* src, size_t pitch, bool vec, const Quad& q, bool resize,
                                            double ratio_x, double ratio_y, int in_w, int in_h, const Source& source)
{
    // (gathered in a local array and handed over once: values behind a reference would stay in memory until this body is inlined,
    // and the kernels come out with more branches around the same instructions)
    float d[4] = {out[0], out[1], out[2], out[3]};
    if (!resize) {
        const uint8_t* p = src + (size_t)q.row * pitch + (size_t)q.x0 * Source::kBytes;
        if (vec && q.nv == 4) {
            source.four(p, d);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < q.nv) d[k] = source.at(p, k);
        }
    } else {
        int y0, y1;
        float b0, b1;
        tap((int)q.row, ratio_y, in_h, y0, y1, b0, b1);
        const uint8_t* r0 = src + (size_t)y0 * pitch;
        const uint8_t* r1 = src + (size_t)y1 * pitch;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < q.nv) {
                int s0, s1;
                float a0, a1;
                tap(q.x0 + k, ratio_x, in_w, s0, s1, a0, a1);
                const float h0 = source.at(r0, s0) * a0 + source.at(r0, s1) * a1;
                const float h1 = source.at(r1, s0) * a0 + source.at(r1, s1) * a1;
                d[k] = h0 * b0 + h1 * b1;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = d[k];
}

// a float32 plane as a source: value(x) of every source value x, applied before the filter; vec: one 16-byte load
template <class Value>
struct PlaneSource {
    static constexpr size_t kBytes = 4;
    Value value;
    __device__ __forceinline__ float at(const uint8_t* p, int x) const { return value(reinterpret_cast<const float*>(p)[x]); }
    __device__ __forceinline__ void four(const uint8_t* p, float (&d)[4]) const
    {
        const float4 v = *reinterpret_cast<const float4*>(p);
        d[0] = value(v.x); d[1] = value(v.y); d[2] = value(v.z); d[3] = value(v.w);
    }
};

template <class Value>
__device__ __forceinline__ void quad_values(float (&d)[4], const uint8_t* src, size_t pitch, bool vec, const Quad& q, bool resize,
                                            double ratio_x, double ratio_y, int in_w, int in_h, Value value)
{
    quad_gather(d, src, pitch, vec, q, resize, ratio_x, ratio_y, in_w, in_h, PlaneSource<Value>{value});
}

// The tail of the code kernels on a quad's values: clip (d keeps the clipped values), code, 12 bytes of codes and, where the call
// has depth planes, the four clipped values.
__device__ __forceinline__ void codes_out(float (&d)[4], const Quad& q, const DepthCodesArgs& a)
{
    uint32_t px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        d[k] = clip_np(d[k], a.fmax);
        px[k] = pixel(d[k], a.multi, a.bgr);
    }
    store_pixels(a.codes + q.f * a.codes_stride + (size_t)q.row * a.codes_pitch + (size_t)q.x0 * 3u, px, q.nv, a.codes_vec);
    if (a.plane) store_plane(reinterpret_cast<float*>(a.plane + q.f * a.plane_stride + (size_t)q.row * a.plane_pitch) + q.x0, d, q.nv, a.plane_vec);
}

}  // namespace depth_code
}  // namespace mdvt
