// mdvt_msaa_common.h -- the pieces of the key-plane render (mdvt_msaa.hip) that the near-plane clipping render
// (mdvt_near_clip.hip) shares: sample positions, vertex and colour loads, edge values, the per-row column range and the resolve.
// Included inside nothing: it opens the grid namespace itself (one copy per sub-pixel grid, mdvt_internal.h).
#pragma once

#include "mdvt_device.h"

namespace mdvt {
namespace MDVT_GRID {

namespace {

constexpr int kMsaaTPB = 256;
constexpr int kMsaaSmallBox = 16;    // pixels in the box of a triangle that is walked whole (every pixel, every sample)

// Sample offsets inside the pixel in 1/16 px, four nibbles (sample k = bits 4k..4k+3), x and y per pattern.
constexpr uint32_t kPatX[2] = {0xA2E6u, 0x6DA3u};    // (6, 14, 2, 10), (3, 10, 13, 6)
constexpr uint32_t kPatY[2] = {0xEA62u, 0x36DAu};    // (2, 6, 10, 14), (10, 13, 6, 3)
__device__ __forceinline__ int sample_ox(int pattern, int k) { return (int)((kPatX[pattern] >> (4 * k)) & 15u) * (kSubpix / 16); }
__device__ __forceinline__ int sample_oy(int pattern, int k) { return (int)((kPatY[pattern] >> (4 * k)) & 15u) * (kSubpix / 16); }

// Vertex (i, j) of frame `fr` for one eye: decode, grid position, vertex programme (the general paths' functions).
__device__ __forceinline__ Vert msaa_vertex(const MsaaArgs& a, const FrameDev& f, int fr, int eye, int i, int j)
{
    const uint8_t* row = a.depth + (size_t)fr * a.depth_stride + (size_t)i * a.depth_pitch;
    const float z = decode_z(code16_of(load_px_bytes(row, j)), f.mult, f.scale);
    const float gx = (float)j * f.sx, gy = (float)i * f.sy;
    float xc = 0.0f, yc = 0.0f;
    if (f.general) camera_point(f, gx, gy, z, xc, yc);
    return vertex_for_eye(f, eye, gx, gy, z, xc, yc);
}

__device__ __forceinline__ uint32_t msaa_colour(const MsaaArgs& a, int fr, int i, int j)
{
    return load_px_bytes(a.color + (size_t)fr * a.color_stride + (size_t)i * a.color_pitch, j);
}

__device__ __forceinline__ void edge_values(const TriSetup& t, int X, int Y, i64& w0, i64& w1, i64& w2)
{
    w0 = mul64(t.dx0, Y - t.by0) - mul64(t.dy0, X - t.bx0);
    w1 = mul64(t.dx1, Y - t.by1) - mul64(t.dy1, X - t.bx1);
    w2 = mul64(t.dx2, Y - t.by2) - mul64(t.dy2, X - t.bx2);
}

// One sample position against the triangle; on a hit, posts the fragment's key.
__device__ __forceinline__ void msaa_post(const TriSetup& t, float ra, int X, int Y, u64 draw, unsigned long long* word)
{
    i64 w0, w1, w2;
    edge_values(t, X, Y, w0, w1, w2);
    if (!(edge_in(w0, t.dx0, t.dy0) && edge_in(w1, t.dx1, t.dy1) && edge_in(w2, t.dx2, t.dy2))) return;
    const float q0 = ((float)w0 * ra) * t.iz0, q1 = ((float)w1 * ra) * t.iz1, q2 = ((float)w2 * ra) * t.iz2;
    const float iz = (q0 + q1) + q2;
    atomicMin(word, ((u64)depth_bits(iz) << 32) | draw);
}

// Columns [lo, hi] of pixels whose sample at (px S + ox, Y) may lie inside the triangle: each orientation-normalised edge
// w = dx (Y - by) - dy (X - bx) >= 0 bounds X from above (dy > 0) or below (dy < 0).  f64 estimate (good to far below a pixel
// across the whole snap range), widened by one pixel.  false: the row holds no sample of the triangle.
__device__ __forceinline__ bool sample_row_range(const TriSetup& t, int Y, int ox, int px0, int px1, int& lo, int& hi)
{
    double xlo = -1.0e300, xhi = 1.0e300;
    const int dxs[3] = {t.dx0, t.dx1, t.dx2}, dys[3] = {t.dy0, t.dy1, t.dy2};
    const int bxs[3] = {t.bx0, t.bx1, t.bx2}, bys[3] = {t.by0, t.by1, t.by2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double A = (double)mul64(dxs[k], Y - bys[k]);
        if (dys[k] == 0) { if (A < 0.0) return false; continue; }
        const double x = (double)bxs[k] + A / (double)dys[k];
        if (dys[k] > 0) xhi = fmin(xhi, x); else xlo = fmax(xlo, x);
    }
    const double l = floor((xlo - (double)ox) / (double)kSubpix) - 1.0, h = floor((xhi - (double)ox) / (double)kSubpix) + 1.0;
    lo = l < (double)px0 ? px0 : (l > (double)px1 ? px1 + 1 : (int)l);
    hi = h > (double)px1 ? px1 : (h < (double)px0 ? px0 - 1 : (int)h);
    return lo <= hi;
}

__device__ __forceinline__ uint32_t resolve_channel(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, int rule)
{
    if (rule) return ((((s0 + s1 + 1u) >> 1) + ((s2 + s3 + 1u) >> 1) + 1u) >> 1);
    return (s0 + s1 + s2 + s3 + 2u) >> 2;
}

}  // namespace

}  // namespace MDVT_GRID
}  // namespace mdvt
