// mdvt_msaa.hip -- opt-in 4x multisampled render (mdvt_config.samples = 4), mesh and points, every kind of frame.
//
// What a GL does with a 4x multisampled framebuffer, restated with the decree's vertex programme, snap, fill rule and shading
// arithmetic (the oracle's candidate orc_render_stereo_gl(samples = 4) is the specification, held bit for bit):
//   * coverage and depth per SAMPLE: the fill rule of edge_in at each of the four sample positions (pattern 0: the Direct3D /
//     Vulkan standard (6,2) (14,6) (2,10) (10,14) / 16 px, 1: SwiftShader's (3,10) (10,13) (13,6) (6,3) / 16, image space, y down),
//     1/Z of the sample = ((f32(w_k) ra) iz_k) summed (q0 + q1) + q2;
//   * colour ONCE per pixel, at the pixel centre, even where the centre lies outside the triangle (no centroid sampling); with
//     izc <= 0 the plain linear combination;
//   * the nearest fragment keeps a sample, an exact tie goes to the first drawn (all tri1 row-major, then all tri2; points: the
//     lower source index, its two triangles in order);
//   * resolve 0: (s0 + s1 + s2 + s3 + 2) >> 2, resolve 1: SwiftShader's avg(avg(s0, s1), avg(s2, s3)), avg = (a + b + 1) >> 1;
//     an uncovered sample holds the key colour; hole = resolved colour == key colour, a hole's RGB is written as 0.
//
// Two kernels per launch set, on one stream:
//   k_msaa_raster   one lane per triangle (points: per point, its two triangles); posts one 64-bit atomicMin per covered sample
//                   into the key plane [slot][eye][H*W][4]: ~bits(1/Z) << 32 | draw id, so the minimum is "nearest, then first
//                   drawn" and no tie pass is needed.  A triangle with a box of more than kMsaaSmallBox pixels walks, per pixel
//                   row and sample, only the columns its three edges leave open (estimated in f64, widened by a pixel; the
//                   exact integer test decides).
//   k_msaa_resolve  one lane per pixel: re-derives the (at most four distinct) winning triangles from the source frame, shades
//                   each once at the pixel centre, resolves, writes RGB, mask and hole counts, and empties the key words again.
// None of the single-sample kernels is used or changed; the vertex bits come from the same mdvt_device.h functions.
#include "mdvt_msaa_common.h"

namespace mdvt {
namespace MDVT_GRID {      // one copy per sub-pixel grid (mdvt_internal.h)

namespace {

// One triangle of the draw order, ready to rasterise or shade.  Mesh: draw = pass * ncell + i * (W - 1) + j (dmt:1243-1254);
// points: draw = 2 k + t, triangle t of the unit square around the snapped vertex k (the oracle's two triangles, at the
// vertex's depth, never culled).  Returns false for a triangle that draws nothing (removed, behind the near plane, degenerate,
// culled).  p[3]: the vertex colours.
__device__ bool msaa_triangle(const MsaaArgs& a, const FrameDev& f, int fr, int slot, int eye, uint32_t draw, TriSetup& t, uint32_t (&p)[3])
{
    const int W = a.W, H = a.H;
    if (a.mode == MDVT_MODE_MESH) {
        const uint32_t ncell = (uint32_t)(W - 1) * (uint32_t)(H - 1);
        if (a.tri_invalid && a.tri_invalid[(size_t)slot * a.ws_stride_tri + draw]) return false;      // dmt:1372
        const int pass = draw >= ncell ? 1 : 0;
        const uint32_t cell = draw - (pass ? ncell : 0u);
        const int i = (int)(cell / (uint32_t)(W - 1)), j = (int)(cell % (uint32_t)(W - 1));
        // v0 = (i, j); (v1, v2) = (i+1, j), (i+1, j+1) for tri1, (i+1, j+1), (i, j+1) for tri2
        const int vi[3] = {i, i + 1, pass ? i : i + 1};
        const int vj[3] = {j, pass ? j + 1 : j, j + 1};
        int X[3], Y[3];
        float iz[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const Vert v = msaa_vertex(a, f, fr, eye, vi[k], vj[k]);
            X[k] = snap(v.u); Y[k] = snap(v.v);
            iz[k] = v.ok ? rcp_exact(v.z) : 0.0f;
            p[k] = msaa_colour(a, fr, vi[k], vj[k]);
        }
        return tri_setup_snapped(t, X[0], Y[0], iz[0], X[1], Y[1], iz[1], X[2], Y[2], iz[2], a.cull);
    }
    const uint32_t k = draw >> 1;
    const int i = (int)(k / (uint32_t)W), j = (int)(k % (uint32_t)W);
    if (a.unused && a.unused[(size_t)slot * a.ws_stride_px + k]) return false;                       // dmt:1091
    const Vert v = msaa_vertex(a, f, fr, eye, i, j);
    if (!v.ok) return false;
    const float hs = 0.5f;
    const float cu = (float)snap(v.u) / (float)kSubpix, cv = (float)snap(v.v) / (float)kSubpix;
    const float iz = rcp_exact(v.z);
    p[0] = p[1] = p[2] = msaa_colour(a, fr, i, j);
    if ((draw & 1u) == 0u)
        return tri_setup_snapped(t, snap(cu - hs), snap(cv - hs), iz, snap(cu - hs), snap(cv + hs), iz, snap(cu + hs), snap(cv + hs), iz, 0);
    return tri_setup_snapped(t, snap(cu - hs), snap(cv - hs), iz, snap(cu + hs), snap(cv + hs), iz, snap(cu + hs), snap(cv - hs), iz, 0);
}

// grid: (triangles / kMsaaTPB, eye, frame slot).  Mesh: one lane per triangle; points: one lane per point.
__global__ void __launch_bounds__(kMsaaTPB) k_msaa_raster(const MsaaArgs a)
{
    const int W = a.W, H = a.H;
    const int eye = (int)blockIdx.y, slot = (int)blockIdx.z, fr = a.frame0 + slot;
    const uint32_t id = blockIdx.x * (uint32_t)kMsaaTPB + threadIdx.x;
    const uint32_t nitems = a.mode == MDVT_MODE_MESH ? 2u * (uint32_t)(W - 1) * (uint32_t)(H - 1) : (uint32_t)W * (uint32_t)H;
    if (id >= nitems) return;
    const FrameDev& f = a.fp[fr];
    const size_t npx = (size_t)W * (size_t)H;
    unsigned long long* keys = a.keys + ((size_t)slot * 2 + (size_t)eye) * npx * 4;
    const int ntris = a.mode == MDVT_MODE_MESH ? 1 : 2;
    for (int tt = 0; tt < ntris; ++tt) {
        const uint32_t draw = a.mode == MDVT_MODE_MESH ? id : 2u * id + (uint32_t)tt;
        TriSetup t;
        uint32_t p[3];
        if (!msaa_triangle(a, f, fr, slot, eye, draw, t, p)) continue;
        const int px0 = max(0, floordiv_subpix(t.minX) - 1), px1 = min(W - 1, floordiv_subpix(t.maxX) + 1);
        const int py0 = max(0, floordiv_subpix(t.minY) - 1), py1 = min(H - 1, floordiv_subpix(t.maxY) + 1);
        if (px0 > px1 || py0 > py1) continue;
        const float ra = rcp_exact((float)t.area2);
        const bool whole = (px1 - px0 + 1) * (py1 - py0 + 1) <= kMsaaSmallBox;      // (W H < 2^31: mdvt_api_render.hip)
        for (int py = py0; py <= py1; ++py) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ox = sample_ox(a.pattern, k), Y = py * kSubpix + sample_oy(a.pattern, k);
                int lo = px0, hi = px1;
                if (!whole && !sample_row_range(t, Y, ox, px0, px1, lo, hi)) continue;
                for (int px = lo; px <= hi; ++px)
                    msaa_post(t, ra, px * kSubpix + ox, Y, draw, keys + ((size_t)py * W + (size_t)px) * 4 + k);
            }
        }
    }
}

// The colour of triangle `draw` at the centre of pixel (x, y): rint(((q0 c0 + q1 c1) + q2 c2) * (1 / izc)), or the plain linear
// combination where izc <= 0 (the centre far outside the triangle), clamped to [0, 255], NaN -> 0 (shade_px).
__device__ uint32_t msaa_shade(const MsaaArgs& a, const FrameDev& f, int fr, int slot, int eye, uint32_t draw, int x, int y)
{
    TriSetup t;
    uint32_t p[3];
    if (!msaa_triangle(a, f, fr, slot, eye, draw, t, p)) return a.key_rgb;     // (cannot happen: the triangle posted the key)
    i64 c0, c1, c2;
    edge_values(t, x * kSubpix + kSubpix / 2, y * kSubpix + kSubpix / 2, c0, c1, c2);
    const float ra = rcp_exact((float)t.area2);
    const float l0 = (float)c0 * ra, l1 = (float)c1 * ra, l2 = (float)c2 * ra;
    const float q0 = l0 * t.iz0, q1 = l1 * t.iz1, q2 = l2 * t.iz2;
    const float izc = (q0 + q1) + q2;
    if (izc > 0.0f) return shade_px(q0, q1, q2, rcp_exact(izc), p[0], p[1], p[2]);
    return shade_px(l0, l1, l2, 1.0f, p[0], p[1], p[2]);                        // (num * 1 == num: the unscaled combination)
}

// grid: (pixels / kMsaaTPB, eye, frame slot)
__global__ void __launch_bounds__(kMsaaTPB) k_msaa_resolve(const MsaaArgs a)
{
    const int W = a.W, H = a.H;
    const int eye = (int)blockIdx.y, slot = (int)blockIdx.z, fr = a.frame0 + slot;
    const size_t npx = (size_t)W * (size_t)H;
    const size_t o = (size_t)blockIdx.x * kMsaaTPB + threadIdx.x;
    bool hole = false;
    if (o < npx) {
        const FrameDev& f = a.fp[fr];
        const int y = (int)(o / (size_t)W), x = (int)(o % (size_t)W);
        unsigned long long* kw = a.keys + ((size_t)slot * 2 + (size_t)eye) * npx * 4 + o * 4;
        u64 key[4];
        uint32_t col[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) key[k] = kw[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            col[k] = a.key_rgb;
            if (key[k] == kEmpty64) continue;
            const uint32_t draw = (uint32_t)key[k];
            bool seen = false;
#pragma unroll
            for (int q = 0; q < k; ++q)
                if (!seen && key[q] != kEmpty64 && (uint32_t)key[q] == draw) { col[k] = col[q]; seen = true; }
            if (!seen) col[k] = msaa_shade(a, f, fr, slot, eye, draw, x, y);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) kw[k] = kEmpty64;      // the EMPTY invariant for the next use of the slot
        uint32_t rgb = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int sh = 8 * ch;
            rgb |= resolve_channel((col[0] >> sh) & 0xFFu, (col[1] >> sh) & 0xFFu, (col[2] >> sh) & 0xFFu, (col[3] >> sh) & 0xFFu,
                                   a.resolve) << sh;
        }
        hole = rgb == a.key_rgb;
        store_px_bytes(a.rgb[eye] + (size_t)fr * a.rgb_stride + (size_t)y * a.rgb_pitch, x, hole ? 0u : rgb);
        a.mask[eye][(size_t)fr * a.mask_stride + (size_t)y * a.mask_pitch + (size_t)x] = hole ? 255 : 0;
    }
    if (a.hole_counts) {
        const u64 b = __ballot(hole);
        if ((threadIdx.x & (warpSize - 1)) == 0 && b) atomicAdd(&a.hole_counts[2 * (size_t)fr + (size_t)eye], (uint32_t)__popcll(b));
    }
}

}  // namespace

hipError_t launch_msaa_render(const MsaaArgs& a, int n, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    const size_t npx = (size_t)a.W * (size_t)a.H;
    const size_t items = a.mode == MDVT_MODE_MESH ? 2 * (size_t)(a.W - 1) * (size_t)(a.H - 1) : npx;
    hipLaunchKernelGGL(k_msaa_raster, dim3((unsigned)((items + kMsaaTPB - 1) / kMsaaTPB), 2, (unsigned)n), dim3(kMsaaTPB), 0, s, a);
    hipLaunchKernelGGL(k_msaa_resolve, dim3((unsigned)((npx + kMsaaTPB - 1) / kMsaaTPB), 2, (unsigned)n), dim3(kMsaaTPB), 0, s, a);
    return hipGetLastError();
}

}  // namespace MDVT_GRID
}  // namespace mdvt
