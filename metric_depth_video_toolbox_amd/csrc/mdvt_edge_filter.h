// mdvt_edge_filter.h -- the device functions of the 89-degree oblique-triangle filter (dmt:1283-1294, 1339-1344): the exact test, its
// two screens and the verdict on both triangles of a cell.  One place for the kernels that filter: k_edge_filter[4]
// (mdvt_edge_filter.hip) and the geometry export (mdvt_geometry.hip).  Compiled with -ffp-contract=off (mdvt_device.h).
#pragma once

#include "mdvt_device.h"

namespace mdvt {

// =================================================================================================
// 89-degree oblique-triangle filter (dmt:1283-1294, 1339-1344), f64 exactly as NumPy >= 2 evaluates it
// =================================================================================================

__device__ __forceinline__ bool tri_oblique(const double (&a)[3], const double (&b)[3], const double (&c)[3])
{
    const double e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const double e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    const double nx = e1y * e2z - e1z * e2y;
    const double ny = e1z * e2x - e1x * e2z;
    const double nz = e1x * e2y - e1y * e2x;
    const double vx = -((a[0] + b[0]) + c[0]) / 3.0;
    const double vy = -((a[1] + b[1]) + c[1]) / 3.0;
    const double vz = -((a[2] + b[2]) + c[2]) / 3.0;
    const double dot = (nx * vx + ny * vy) + nz * vz;
    const double len_n = sqrt((nx * nx + ny * ny) + nz * nz);
    const double len_v = sqrt((vx * vx + vy * vy) + vz * vz);
    const double cosine = dot / (len_n * len_v + 1e-15);
    return cosine < 0x1.1df0b2b89dd37p-6;          // np.cos(np.radians(89.0))
}

// Division-free screening of the same test.  cos < c0  <=>  dot < c0 * (|n||v| + 1e-15); with the
// unnormalised view vector vs = a+b+c (v = -vs/3) this is  -n.vs < c0 * |n| |vs|  up to the 1e-15 term.
// Squaring removes the square roots.  The screening value carries ~1e-15 relative rounding error and
// ignores the 1e-15 term, which moves the threshold by the relative amount 1e-15 / (|n||v|): a triangle with
// |n||v| < 1e-8 (content nearer than ~0.3 m at 1080p: tiny triangles, tiny view vectors) is therefore NOT
// decided here, nor is one whose margin is below kScreenMargin (5e-7 in linear terms, against <= 1e-7 from the
// dropped term); both go through the exact formula.  Everything else provably gets the exact formula's decision.
constexpr double kScreenMargin = 1e-6;
constexpr double kScreenMinNNSS = 9e-16;          // (3 |n||v|)^2 for |n||v| = 1e-8

// returns 0 = valid, 1 = oblique (removed), 2 = undecided
__device__ __forceinline__ int tri_oblique_screen(const double (&a)[3], const double (&b)[3], const double (&c)[3])
{
    const double e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const double e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    // (explicit fused multiply-adds: the screen only has to be accurate, not bit-identical to anything, and the
    //  filter is bound by the f64 VALU rate -- the exact path below keeps the decree's one-rounding-per-node form)
    const double nx = fma(e1y, e2z, -(e1z * e2y));
    const double ny = fma(e1z, e2x, -(e1x * e2z));
    const double nz = fma(e1x, e2y, -(e1y * e2x));
    const double sx = (a[0] + b[0]) + c[0], sy = (a[1] + b[1]) + c[1], sz = (a[2] + b[2]) + c[2];
    const double d = -fma(nz, sz, fma(ny, sy, nx * sx));               // 3 * dot
    const double nn = fma(nz, nz, fma(ny, ny, nx * nx));
    const double ss = fma(sz, sz, fma(sy, sy, sx * sx));               // 9 * |v|^2
    const double c0 = 0x1.1df0b2b89dd37p-6;
    const double rhs = (c0 * c0) * (nn * ss);                          // (c0 |n| |vs|)^2
    if (!(nn * ss > kScreenMinNNSS)) return 2;                         // degenerate / zero depth / tiny: exact path
    const double lhs = d * fabs(d);                                    // signed square
    const double tol = kScreenMargin * rhs;
    if (lhs < rhs - tol) return 1;
    if (lhs > rhs + tol) return 0;
    return 2;
}

// f32 pre-screen of the same test (r04), from the closed form of a triangle whose vertices are P_k = z_k (u_k, v_k, 1) on the
// grid's rays u in {a, a + px}, v in {b, b + py}:  n = (P1 - P0) x (P2 - P0) and n . P_k = z0 z1 z2 det(r0, r1, r2) = -px py z0 z1 z2
// for both triangles of a cell, so with s = P0 + P1 + P2 (the view vector is -s / 3)
//     3 dot = -n . s = 3 px py z0 z1 z2 > 0,    tri1 (A, B, C): nx = py zA (zC - zB), ny = px zC (zB - zA),
//                                               tri2 (A, C, D): nx = py zC (zD - zA), ny = px zA (zC - zD),
//     nz = -(a nx + b ny) - px py z1 z2   (from n . P0),
// and the test cos < cos 89 is  (3 dot)^2 < c0^2 |n|^2 |s|^2.  No difference of nearly equal PRODUCTS is left (the generic
// cross product of the edge vectors cancels ~4 digits): every factor is an input or one f32 subtraction of inputs, |n|^2 and
// |s|^2 are sums of squares, and nz's one cancellation is bounded by eps (|a nx| + |b ny| + ...) <= eps (|a| + |b| + 1) |n|.
// With |a|, |b| <= 64 both sides are good to ~1e-5 relative in f32, the f64 formula of the reference's order differs from
// the exact value by ~1e-15, its 1e-15 term moves the threshold by < 1e-7 when (3 |n||v|)^2 > 9e-16: a margin of 1e-3
// decides the same way for sure.  The rest -- a fraction of a per cent of the triangles -- takes the f64 screen and, inside
// its own margin, the exact formula.  returns 0 = valid, 1 = oblique (removed), 2 = undecided
__device__ __forceinline__ int tri_oblique_screen_f32(float a, float b, float pp, float z0, float t12 /* pp z1 z2 */,
                                                      float nx, float ny, float sx, float sy, float sz)
{
    // (explicit fused multiply-adds: the screen only has to be accurate, not bit-identical to anything)
    const float nz = -__builtin_fmaf(a, nx, __builtin_fmaf(b, ny, t12));
    const float nn = __builtin_fmaf(nz, nz, __builtin_fmaf(ny, ny, nx * nx));
    const float ss = __builtin_fmaf(sz, sz, __builtin_fmaf(sy, sy, sx * sx));
    const float d3 = (3.0f * z0) * t12;
    const float lhs = d3 * d3;
    const float nnss = nn * ss;
    const float rhs = 0x1.3f61d0p-12f * nnss;                           // cos^2 89 degrees (f32: 6e-8 relative, inside the margin)
    // (no branches: 0 = valid, 1 = oblique (removed), 2 = undecided -- degenerate / zero depth / tiny / NaN / inside the margin)
    const bool ok = nnss > 1.0e-15f;
    const bool rem = ok && lhs < rhs * 0.999f, val = ok && lhs > rhs * 1.001f;
    return rem ? 1 : (val ? 0 : 2);
}

struct CellRaysF32 { float a, a1, b, b1, px, py; bool ok; };     // the f32 pre-screen's view of the cell's rays (ok: all within +-64)
__device__ __forceinline__ CellRaysF32 cell_rays_f32(double x0r, double x1r, double y0r, double y1r)
{
    CellRaysF32 r;
    r.a = (float)x0r; r.b = (float)y0r; r.a1 = (float)x1r; r.b1 = (float)y1r;
    r.px = (float)(x1r - x0r); r.py = (float)(y1r - y0r);
    r.ok = fabsf(r.a) <= 64.0f && fabsf(r.b) <= 64.0f && fabsf(r.a1) <= 64.0f && fabsf(r.b1) <= 64.0f;
    return r;
}

// f32 pre-screen of both triangles of a cell: s1 | s2 << 2, each 0 = valid, 1 = oblique (removed), 2 = undecided
__device__ __forceinline__ uint32_t edge_filter_prescreen(const CellRaysF32& r, float zA, float zB, float zC, float zD)
{
    if (!r.ok) return 2u | (2u << 2);
    // tri1 = (A, B, C) = rays (a, b), (a, b'), (a', b');  tri2 = (A, C, D) = (a, b), (a', b'), (a', b)
    const float pp = r.px * r.py;
    const int s1 = tri_oblique_screen_f32(r.a, r.b, pp, zA, (pp * zB) * zC, (r.py * zA) * (zC - zB), (r.px * zC) * (zB - zA),
                                          __builtin_fmaf(r.a1, zC, r.a * (zA + zB)), __builtin_fmaf(r.b1, zB + zC, r.b * zA), (zA + zB) + zC);
    const int s2 = tri_oblique_screen_f32(r.a, r.b, pp, zA, (pp * zC) * zD, (r.py * zC) * (zD - zA), (r.px * zA) * (zC - zD),
                                          __builtin_fmaf(r.a1, zC + zD, r.a * zA), __builtin_fmaf(r.b1, zC, r.b * (zA + zD)), (zA + zC) + zD);
    return (uint32_t)s1 | ((uint32_t)s2 << 2);
}

// Both triangles of cell (i, j): bit 0 = tri1 (A, B, C) removed, bit 1 = tri2 (A, C, D) removed.  `pre` = edge_filter_prescreen's
// verdict; x0r.. are the cell's ray coordinates (g - c) * (1 / f) in f64 (the f64 screen; the exact path recomputes the vertices
// in the reference's own order).
__device__ __forceinline__ uint32_t edge_filter_cell(const FrameDev& f, int i, int j, int of_by_one, double x0r, double x1r, double y0r,
                                                     double y1r, uint32_t pre, float zA, float zB, float zC, float zD)
{
    int s1 = (int)(pre & 3u), s2 = (int)(pre >> 2);
    if (s1 == 2 || s2 == 2) {
        asm volatile("; f64 screen" ::: "memory");
        const double dA = (double)zA, dB = (double)zB, dC = (double)zC, dD = (double)zD;
        const double A[3] = {x0r * dA, y0r * dA, dA};
        const double B[3] = {x0r * dB, y1r * dB, dB};
        const double Cc[3] = {x1r * dC, y1r * dC, dC};
        const double D[3] = {x1r * dD, y0r * dD, dD};
        if (s1 == 2) s1 = tri_oblique_screen(A, B, Cc);      // tri1 = (v[i,j], v[i+1,j], v[i+1,j+1])
        if (s2 == 2) s2 = tri_oblique_screen(A, Cc, D);      // tri2 = (v[i,j], v[i+1,j+1], v[i,j+1])
    }
    if (s1 == 2 || s2 == 2) {
        // exact path: the reference's own evaluation order (dmt:1127-1128, 1283-1294)
        double Ae[3], Be[3], Ce[3], De[3];
        vertex_f64(f, i, j, of_by_one, zA, Ae);
        vertex_f64(f, i + 1, j, of_by_one, zB, Be);
        vertex_f64(f, i + 1, j + 1, of_by_one, zC, Ce);
        vertex_f64(f, i, j + 1, of_by_one, zD, De);
        if (s1 == 2) s1 = tri_oblique(Ae, Be, Ce) ? 1 : 0;
        if (s2 == 2) s2 = tri_oblique(Ae, Ce, De) ? 1 : 0;
    }
    return (s1 == 1 ? 1u : 0u) | (s2 == 1 ? 2u : 0u);
}

}  // namespace mdvt
