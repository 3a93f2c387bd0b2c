// mdvt_telea_common.h -- the parts of Telea's estimate (cv2.inpaint INPAINT_TELEA, radius 3) that the level-synchronous
// completion (k_telea_fill, mdvt_telea_levels.hip) and the heap-order completion (k_telea_heap, mdvt_telea_heap.hip) share: the
// quadrant solve of FastMarching_solve, the read set of an estimate, the disc with its distance factors and the estimate of
// one pixel from its 9 x 9 neighbourhood in LDS.  One copy of the arithmetic, so that both orders are bit-exact against the
// same oracle expressions (orc_telea_pixel).
#pragma once
#include "mdvt_device.h"

namespace mdvt {

// OpenCV's FastMarching_solve for one quadrant: k = the neighbour is known (in the image, filled before this level), t = its T.
__device__ __forceinline__ float telea_solve(bool k1, float t1, bool k2, float t2)
{
    const double a11 = k1 ? (double)t1 : 1.0e6, a22 = k2 ? (double)t2 : 1.0e6;
    const double m12 = a11 < a22 ? a11 : a22;
    double sol;
    if (k1) {
        if (k2) sol = fabs(a11 - a22) >= 1.0 ? 1.0 + m12 : (a11 + a22 + sqrt(2.0 - (a11 - a22) * (a11 - a22))) * 0.5;
        else sol = 1.0 + a11;
    } else if (k2) sol = 1.0 + a22;
    else sol = 1.0 + m12;
    return (float)sol;
}

// What the estimate of a pixel reads: the radius-3 disc and the 4-neighbours of its pixels (57 offsets, all within an L1
// distance of 5: the level of any of them differs from the pixel's own by at most 5).
struct NeedOffsets { int8_t dx[64], dy[64]; int n; };
constexpr NeedOffsets make_need_offsets()
{
    NeedOffsets t{};
    int n = 0;
    for (int dy = -4; dy <= 4; ++dy)
        for (int dx = -4; dx <= 4; ++dx) {
            const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
            if (ax + ay > 5 || (ax == 4 && ay > 1) || (ay == 4 && ax > 1) || (ax == 0 && ay == 0)) continue;
            t.dx[n] = (int8_t)dx; t.dy[n] = (int8_t)dy; ++n;
        }
    t.n = n;
    return t;
}
__device__ __constant__ const NeedOffsets kNeedOffsets = make_need_offsets();

// The radius-3 disc without its centre, in the oracle's row-major order (28 pixels): offset (dx, dy) and the distance factor
// (float)(1.0 / (vl * sqrt(vl))), vl = dx^2 + dy^2 -- six distinct values, written out (f64 arithmetic, rounded once to f32).
struct DiscPixel { float dx, dy, dst; int cell; };             // cell = index of the pixel in the 9 x 9 neighbourhood
#define MDVT_DISC(dx, dy, dst) {(float)(dx), (float)(dy), dst, ((dy) + 4) * 9 + (dx) + 4}
#define MDVT_D1 0x1.000000p+0f
#define MDVT_D2 0x1.6a09e6p-2f
#define MDVT_D4 0x1.000000p-3f
#define MDVT_D5 0x1.6e5b7ep-4f
#define MDVT_D8 0x1.6a09e6p-5f
#define MDVT_D9 0x1.2f684cp-5f
__device__ __constant__ const DiscPixel kDisc[32] = {
    MDVT_DISC(0, -3, MDVT_D9),
    MDVT_DISC(-2, -2, MDVT_D8), MDVT_DISC(-1, -2, MDVT_D5), MDVT_DISC(0, -2, MDVT_D4), MDVT_DISC(1, -2, MDVT_D5), MDVT_DISC(2, -2, MDVT_D8),
    MDVT_DISC(-2, -1, MDVT_D5), MDVT_DISC(-1, -1, MDVT_D2), MDVT_DISC(0, -1, MDVT_D1), MDVT_DISC(1, -1, MDVT_D2), MDVT_DISC(2, -1, MDVT_D5),
    MDVT_DISC(-3, 0, MDVT_D9), MDVT_DISC(-2, 0, MDVT_D4), MDVT_DISC(-1, 0, MDVT_D1), MDVT_DISC(1, 0, MDVT_D1), MDVT_DISC(2, 0, MDVT_D4), MDVT_DISC(3, 0, MDVT_D9),
    MDVT_DISC(-2, 1, MDVT_D5), MDVT_DISC(-1, 1, MDVT_D2), MDVT_DISC(0, 1, MDVT_D1), MDVT_DISC(1, 1, MDVT_D2), MDVT_DISC(2, 1, MDVT_D5),
    MDVT_DISC(-2, 2, MDVT_D8), MDVT_DISC(-1, 2, MDVT_D5), MDVT_DISC(0, 2, MDVT_D4), MDVT_DISC(1, 2, MDVT_D5), MDVT_DISC(2, 2, MDVT_D8),
    MDVT_DISC(0, 3, MDVT_D9),
    MDVT_DISC(0, 0, 0.0f), MDVT_DISC(0, 0, 0.0f), MDVT_DISC(0, 0, 0.0f), MDVT_DISC(0, 0, 0.0f)};
#undef MDVT_DISC

constexpr int kRedStride = 36;           // floats between the running sums of one pixel in LDS: 16-byte aligned rows, b128 reads without bank conflicts

// Telea's estimate of one pixel from its 9 x 9 neighbourhood, by one half-wave (lane32 = the lane inside it), with the
// neighbourhood already in LDS: kn = known (in the image and estimated before this pixel), tt = T, cc = colour (0x00BBGGRR),
// cell 40 = the pixel itself.  red: the half-wave's [10][kRedStride] floats of LDS.  dp = kDisc[lane32]; qv, qh = this lane's
// quadrant cells.  on_t(t) receives T of the pixel (the same value in every lane) as soon as it is known; the return value is
// the estimated colour (0x00BBGGRR, in every lane).
// T comes from four lanes solving one quadrant each; every lane weighs its own disc pixel; the 10 running sums (Ia, Jx, Jy per
// channel and the weight) are then added up in the oracle's order j = 0..27 by 10 lanes reading the terms back from LDS -- the
// same left-to-right f32 chain as the oracle's loop, so the result is bit-identical to it.
template <class OnT>
__device__ __forceinline__ uint32_t telea_tile_estimate(const uint8_t* kn, const float* tt, const uint32_t* cc, float (*red)[kRedStride],
                                                        const DiscPixel& dp, int lane32, int qv, int qh, OnT on_t)
{
    constexpr int C0 = 4 * 9 + 4;                      // the pixel itself
    // T of the pixel: FastMarching_solve over the four quadrants, one per lane of a quad; lane 0 keeps it for the levels above
    float t = telea_solve(kn[C0 - 4 + qv] != 0, tt[C0 - 4 + qv], kn[qh] != 0, tt[qh]);
    t = fminf(t, __shfl_xor(t, 1));
    t = fminf(t, __shfl_xor(t, 2));
    on_t(t);
    const bool kxp = kn[C0 + 1] != 0, kxm = kn[C0 - 1] != 0, kyp = kn[C0 + 9] != 0, kym = kn[C0 - 9] != 0;
    const float txp = tt[C0 + 1], txm = tt[C0 - 1], typ = tt[C0 + 9], tym = tt[C0 - 9];
    float gtx, gty;
    if (kxp) gtx = kxm ? (txp - txm) * 0.5f : txp - t;
    else gtx = kxm ? t - txm : 0.0f;
    if (kyp) gty = kym ? (typ - tym) * 0.5f : typ - t;
    else gty = kym ? t - tym : 0.0f;

    // terms of this lane's disc pixel: +Ia (3), -Jx (3), -Jy (3), +s; all 0 where the disc pixel is not known
    float term[10];
#pragma unroll
    for (int c = 0; c < 10; ++c) term[c] = 0.0f;
    const int cell = dp.cell;
    if (lane32 < 28 && kn[cell]) {
        const float rx = -dp.dx, ry = -dp.dy;
        const float lev = (float)(1.0 / (1.0 + fabs((double)(tt[cell] - t))));
        float dir = rx * gtx + ry * gty;
        if (fabsf(dir) <= 0.01f) dir = 0.000001f;
        const float w = fabsf((dp.dst * lev) * dir);
        const bool xp = kn[cell + 1] != 0, xm = kn[cell - 1] != 0, yp = kn[cell + 9] != 0, ym = kn[cell - 9] != 0;
        const uint32_t c0 = cc[cell];
        const uint32_t cxp = xp ? cc[cell + 1] : c0, cxm = xm ? cc[cell - 1] : c0;        // an unknown neighbour stands in as the pixel itself:
        const uint32_t cyp = yp ? cc[cell + 9] : c0, cym = ym ? cc[cell - 9] : c0;        // one-sided and missing differences fall out of a - b
        const float sx = (xp && xm) ? 2.0f : 1.0f, sy = (yp && ym) ? 2.0f : 1.0f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int sh = 8 * ch;
            const int v0 = (c0 >> sh) & 0xFF;
            const int ddx = (int)((cxp >> sh) & 0xFF) - (int)((cxm >> sh) & 0xFF), ddy = (int)((cyp >> sh) & 0xFF) - (int)((cym >> sh) & 0xFF);
            const float gix = (float)ddx * sx, giy = (float)ddy * sy;
            term[ch] = w * (float)v0;              // Ia += .
            term[3 + ch] = -(w * (gix * rx));      // Jx -= .
            term[6 + ch] = -(w * (giy * ry));      // Jy -= .
        }
        term[9] = w;                               // s  += .
    }
#pragma unroll
    for (int c = 0; c < 10; ++c) red[c][lane32] = term[c];
    __builtin_amdgcn_wave_barrier();                   // the half-wave's LDS writes precede its reads (same wave: program order + lgkmcnt)
    float acc = 0.0f;
    if (lane32 < 10) {
        acc = lane32 == 9 ? 1.0e-20f : 0.0f;
        const float4* row = reinterpret_cast<const float4*>(red[lane32]);
#pragma unroll
        for (int j4 = 0; j4 < 7; ++j4) {
            const float4 v = row[j4];
            acc = acc + v.x; acc = acc + v.y; acc = acc + v.z; acc = acc + v.w;      // a term of 0 (pixel not known) leaves acc unchanged, exactly
        }
    }
    __builtin_amdgcn_wave_barrier();
    const int hbase = (threadIdx.x & 63) & 32;         // first lane of this half-wave inside the wave
    const int ch = lane32 < 3 ? lane32 : 0;
    const float Ia = __shfl(acc, hbase + ch), Jx = __shfl(acc, hbase + 3 + ch), Jy = __shfl(acc, hbase + 6 + ch), sw = __shfl(acc, hbase + 9);
    const float jj = Jx * Jx + Jy * Jy;
    const float sat = (float)(((double)(Ia / sw) + (double)(Jx + Jy) / (sqrt((double)jj) + (double)1.0e-20f)) + (double)0.5f);
    float v = rintf(sat);
    if (!(v >= 0.0f)) v = 0.0f;
    if (v > 255.0f) v = 255.0f;
    const uint32_t byte = (uint32_t)v;
    return __shfl(byte, hbase) | (__shfl(byte, hbase + 1) << 8) | (__shfl(byte, hbase + 2) << 16);
}

}  // namespace mdvt
