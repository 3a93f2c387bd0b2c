// mdvt_near_clip.hip -- opt-in near-plane clipping of the mesh (mdvt_set_near_clip(ctx, 1)), one sample or 4x multisampled.
//
// What a GL does with a triangle that crosses its near plane z = 1e-4 (dmt:1520), restated with the decree's vertex programme,
// snap, fill rule and shading (the oracle's candidate orc_render_stereo_gl(near_clip = 1) -- orc_gl_tri / orc_gl_eye_space -- is
// the specification, held bit for bit):
//   * a triangle is clipped when some but not all of its vertices are behind the plane, "behind" being the vertex programme's
//     ok flag (zsrc > near, and Z' > near on general frames), not the sign of Z - near;
//   * a vertex in front keeps the decree's f32 u, v, 1/Z and its colour; each crossing edge P -> Q gets a new vertex, in f64 from
//     the eye-space positions: tt = (zn - P.Z) / (Q.Z - P.Z), u = f32(fxr X / zn + cxr), v likewise, 1/Z = f32(1 / zn), the
//     colour interpolated in f64 and rounded to f32 (not an integer);
//   * the polygon (Sutherland-Hodgman in vertex order, 3 or 4 vertices) is fanned from its first vertex; every fan triangle
//     takes the normal snap, cull test on its own signed area, fill rule and shading (the colour with f32 vertex colours);
//   * draw order: fan triangle f of source triangle d has the id 2 d + f, so ties go to the first drawn as in the GL.
// A crossing edge whose two ends have the same eye-space depth (only a pose that lifts a vertex behind the plane to exactly
// its neighbour's depth) gives tt = +-inf: the new vertex lands at infinity and is clamped by the snap like the oracle's.  Should
// X or Y then be NaN (the two ends also share that coordinate), the oracle converts NaN to an integer, which C leaves undefined;
// such a fan triangle is dropped here.
//
// The key-plane render of mdvt_msaa.hip with a sample count of 1 (the pixel centre) or 4, on one stream:
//   k_clip_detect   (samples 1 only) one lane per vertex and both eyes: flags the (frame, eye) where a vertex behind the plane neighbours one
//                   in front, and zeroes that eye's hole count.  Unflagged eyes keep what the single-sample kernels wrote.
//   k_clip_raster   one lane per source triangle; posts ~bits(1/Z) << 32 | (2 d + f) per covered sample with a 64-bit atomicMin.
//                   A fan triangle with a box of more than kClipWaveBox pixels (a clipped vertex projects from 1e-4 m: wedges
//                   across the frame) is walked by its whole wave, row by row, the lanes across the open columns.
//   k_clip_resolve  one lane per pixel: re-clips the winning source triangles (the clip is a pure function of the three vertices,
//                   nothing is stored per polygon), shades each once at the pixel centre, resolves, writes RGB, mask and counts,
//                   and empties the key words.
// With the flags, raster and resolve leave an unflagged eye at once.  None of the single-sample or 4x kernels is changed.
#include "mdvt_msaa_common.h"

namespace mdvt {
namespace MDVT_GRID {      // one copy per sub-pixel grid (mdvt_internal.h)

namespace {

constexpr int kClipWaveBox = 1024;       // pixels in the box of a fan triangle above which its wave walks it together
// workgroups per (eye, frame slot) of every kernel here, each walking its items in a grid-stride loop: an unflagged eye costs this
// many workgroups that leave at once, not one per 256 triangles (measured: ~23 us per 1080p stereo frame with full grids)
constexpr unsigned kClipBlocks = 512;

struct ClipVert { float u, v, iz; float c[3]; };
struct EyePos { double X, Y, Z; };

// orc_gl_eye_space: vertex (i, j) with source depth z in the render camera's eye space, in f64 (f32 operands promoted).
__device__ __forceinline__ EyePos eye_space(const FrameDev& f, int eye, int i, int j, float z)
{
    const double gx = (double)((float)j * f.sx), gy = (double)((float)i * f.sy), zd = (double)z;
    const double xc = (gx - (double)f.cx) * zd / (double)f.fx, yc = (gy - (double)f.cy) * zd / (double)f.fy;
    EyePos o;
    if (!f.general) {
        const double sign = eye == 0 ? 1.0 : -1.0;
        o.X = xc + sign * ((double)f.dl / (double)f.fxr); o.Y = yc; o.Z = zd;
        return o;
    }
    const float* M = f.M[eye];
    o.X = (M[0] * xc + M[1] * yc) + M[2] * zd + M[3];
    o.Y = (M[4] * xc + M[5] * yc) + M[6] * zd + M[7];
    o.Z = (M[8] * xc + M[9] * yc) + M[10] * zd + M[11];
    return o;
}

__device__ __forceinline__ void colour_floats(uint32_t p, float (&c)[3])
{
    c[0] = (float)(p & 0xFFu); c[1] = (float)((p >> 8) & 0xFFu); c[2] = (float)((p >> 16) & 0xFFu);
}

// Source triangle `src` of the mesh draw order (draw = pass * ncell + i * (W - 1) + j, dmt:1243-1254), clipped against the near
// plane as orc_gl_tri does.  Returns the polygon's vertex count: 0 (removed by the edge filter, or wholly behind the plane), 3
// (wholly in front: the triangle itself, or clipped to a triangle) or 4.
__device__ int clip_source(const MsaaArgs& a, const FrameDev& f, int fr, int slot, int eye, uint32_t src, ClipVert (&pv)[4])
{
    const int W = a.W, H = a.H;
    const uint32_t ncell = (uint32_t)(W - 1) * (uint32_t)(H - 1);
    if (a.tri_invalid && a.tri_invalid[(size_t)slot * a.ws_stride_tri + src]) return 0;      // dmt:1372
    const int pass = src >= ncell ? 1 : 0;
    const uint32_t cell = src - (pass ? ncell : 0u);
    const int i = (int)(cell / (uint32_t)(W - 1)), j = (int)(cell % (uint32_t)(W - 1));
    const int vi[3] = {i, i + 1, pass ? i : i + 1};
    const int vj[3] = {j, pass ? j + 1 : j, j + 1};
    Vert v[3];
    float z[3];
    uint32_t p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint8_t* row = a.depth + (size_t)fr * a.depth_stride + (size_t)vi[k] * a.depth_pitch;
        z[k] = decode_z(code16_of(load_px_bytes(row, vj[k])), f.mult, f.scale);
        const float gx = (float)vj[k] * f.sx, gy = (float)vi[k] * f.sy;
        float xc = 0.0f, yc = 0.0f;
        if (f.general) camera_point(f, gx, gy, z[k], xc, yc);
        v[k] = vertex_for_eye(f, eye, gx, gy, z[k], xc, yc);
        p[k] = msaa_colour(a, fr, vi[k], vj[k]);
    }
    if (!(v[0].ok || v[1].ok || v[2].ok)) return 0;
    if (v[0].ok && v[1].ok && v[2].ok) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            pv[k].u = v[k].u; pv[k].v = v[k].v; pv[k].iz = rcp_exact(v[k].z);
            colour_floats(p[k], pv[k].c);
        }
        return 3;
    }
    EyePos e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = eye_space(f, eye, vi[k], vj[k], z[k]);
    const double zn = (double)kNear;
    int np = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int k1 = k == 2 ? 0 : k + 1;
        if (v[k].ok) {
            pv[np].u = v[k].u; pv[np].v = v[k].v; pv[np].iz = rcp_exact(v[k].z);
            colour_floats(p[k], pv[np].c);
            ++np;
        }
        if (v[k].ok != v[k1].ok) {
            const EyePos& P = e[k];
            const EyePos& Q = e[k1];
            const double tt = (zn - P.Z) / (Q.Z - P.Z);
            const double X = P.X + tt * (Q.X - P.X), Y = P.Y + tt * (Q.Y - P.Y);
            pv[np].u = (float)((double)f.fxr * X / zn + (double)f.cxr);
            pv[np].v = (float)((double)f.fyr * Y / zn + (double)f.cyr);
            pv[np].iz = (float)(1.0 / zn);
            float cp[3], cq[3];
            colour_floats(p[k], cp);
            colour_floats(p[k1], cq);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) pv[np].c[ch] = (float)((double)cp[ch] + tt * ((double)cq[ch] - (double)cp[ch]));
            ++np;
        }
    }
    return np;
}

// Fan triangle `fan` (0 or 1) of a polygon of np vertices: (0, fan + 1, fan + 2), set up with the decree's snap and cull.
__device__ __forceinline__ bool fan_triangle(const ClipVert (&pv)[4], int np, int fan, int cull, TriSetup& t)
{
    t.area2 = 0;
    if (fan + 2 >= np) return false;
    const ClipVert& A = pv[0];
    const ClipVert& B = pv[fan + 1];
    const ClipVert& C = pv[fan + 2];
    if (__builtin_isnan(A.u) || __builtin_isnan(A.v) || __builtin_isnan(B.u) || __builtin_isnan(B.v) ||
        __builtin_isnan(C.u) || __builtin_isnan(C.v))
        return false;                                   // (see the file's head: the oracle is undefined there)
    return tri_setup_snapped(t, snap(A.u), snap(A.v), A.iz, snap(B.u), snap(B.v), B.iz, snap(C.u), snap(C.v), C.iz, cull);
}

template <int NS>
__device__ __forceinline__ int clip_ox(int pattern, int k) { return NS == 1 ? kSubpix / 2 : sample_ox(pattern, k); }
template <int NS>
__device__ __forceinline__ int clip_oy(int pattern, int k) { return NS == 1 ? kSubpix / 2 : sample_oy(pattern, k); }

// Rows py0 + r0, py0 + r0 + rstep, ... of a fan triangle's box; in each row, for each sample, the open columns from lo + c0 in
// steps of cstep.
template <int NS>
__device__ __forceinline__ void clip_walk(const TriSetup& t, float ra, u64 draw, unsigned long long* keys, int W, int pattern,
                                          int px0, int px1, int py0, int py1, bool whole, int c0, int cstep)
{
    for (int py = py0; py <= py1; ++py) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int ox = clip_ox<NS>(pattern, k), Y = py * kSubpix + clip_oy<NS>(pattern, k);
            int lo = px0, hi = px1;
            if (!whole && !sample_row_range(t, Y, ox, px0, px1, lo, hi)) continue;
            for (int px = lo + c0; px <= hi; px += cstep)
                msaa_post(t, ra, px * kSubpix + ox, Y, draw, keys + ((size_t)py * W + (size_t)px) * NS + k);
        }
    }
}

__device__ __forceinline__ void shfl_tri(TriSetup& t, int src)
{
    t.dx0 = __shfl(t.dx0, src); t.dy0 = __shfl(t.dy0, src); t.dx1 = __shfl(t.dx1, src);
    t.dy1 = __shfl(t.dy1, src); t.dx2 = __shfl(t.dx2, src); t.dy2 = __shfl(t.dy2, src);
    t.bx0 = __shfl(t.bx0, src); t.by0 = __shfl(t.by0, src); t.bx1 = __shfl(t.bx1, src);
    t.by1 = __shfl(t.by1, src); t.bx2 = __shfl(t.bx2, src); t.by2 = __shfl(t.by2, src);
    t.minX = __shfl(t.minX, src); t.maxX = __shfl(t.maxX, src); t.minY = __shfl(t.minY, src); t.maxY = __shfl(t.maxY, src);
    t.iz0 = __shfl(t.iz0, src); t.iz1 = __shfl(t.iz1, src); t.iz2 = __shfl(t.iz2, src);
    const uint32_t lo = __shfl((uint32_t)(u64)t.area2, src), hi = __shfl((uint32_t)((u64)t.area2 >> 32), src);
    t.area2 = (i64)(((u64)hi << 32) | lo);
}

// Vertex (i, j) of one eye against its right and lower neighbours: every cell whose corners disagree has such a pair on its border,
// so no straddling triangle goes unflagged (cells removed by the edge filter may be).
__device__ __forceinline__ bool detect_mixed(const MsaaArgs& a, const FrameDev& f, int fr, int eye, int i, int j)
{
    const bool ok = msaa_vertex(a, f, fr, eye, i, j).ok;
    bool mixed = false;
    if (j + 1 < a.W) mixed |= msaa_vertex(a, f, fr, eye, i, j + 1).ok != ok;
    if (i + 1 < a.H) mixed |= msaa_vertex(a, f, fr, eye, i + 1, j).ok != ok;
    return mixed;
}

// grid: (up to kClipBlocks, 1, frame slot), pixels in a grid-stride loop; both eyes per lane (a pure-shift frame's test does not
// depend on the eye: zsrc > near).
__global__ void __launch_bounds__(kMsaaTPB) k_clip_detect(const MsaaArgs a, uint32_t* flags)
{
    const int W = a.W;
    const int slot = (int)blockIdx.z, fr = a.frame0 + slot;
    const FrameDev& f = a.fp[fr];
    const size_t npx = (size_t)W * (size_t)a.H;
    bool mixed[2] = {false, false};
    for (size_t o = (size_t)blockIdx.x * kMsaaTPB + threadIdx.x; o < npx; o += (size_t)gridDim.x * kMsaaTPB) {
        const int i = (int)(o / (size_t)W), j = (int)(o % (size_t)W);
        const bool m0 = detect_mixed(a, f, fr, 0, i, j);
        mixed[0] |= m0;
        mixed[1] |= f.general ? detect_mixed(a, f, fr, 1, i, j) : m0;
    }
#pragma unroll
    for (int eye = 0; eye < 2; ++eye) {
        if (!mixed[eye]) continue;
        flags[2 * slot + eye] = 1u;
        if (a.hole_counts) a.hole_counts[2 * (size_t)fr + (size_t)eye] = 0u;     // (the resolve counts this eye afresh)
    }
}

// Source triangle `id` (past nitems: only to take part in the wave's walks of big fan triangles).
template <int NS>
__device__ __forceinline__ void clip_raster_item(const MsaaArgs& a, const FrameDev& f, int fr, int slot, int eye, uint32_t id,
                                                 uint32_t nitems, unsigned long long* keys)
{
    const int W = a.W, H = a.H;
    ClipVert pv[4];
    const int np = id < nitems ? clip_source(a, f, fr, slot, eye, id, pv) : 0;
    const int lane = (int)(threadIdx.x & (warpSize - 1));
    for (int fan = 0; fan < 2; ++fan) {
        TriSetup t{};
        bool have = fan_triangle(pv, np, fan, a.cull, t);
        int px0 = 0, px1 = -1, py0 = 0, py1 = -1;
        if (have) {
            px0 = max(0, floordiv_subpix(t.minX) - 1); px1 = min(W - 1, floordiv_subpix(t.maxX) + 1);
            py0 = max(0, floordiv_subpix(t.minY) - 1); py1 = min(H - 1, floordiv_subpix(t.maxY) + 1);
            have = px0 <= px1 && py0 <= py1;
        }
        const size_t box = have ? (size_t)(px1 - px0 + 1) * (size_t)(py1 - py0 + 1) : 0;
        const bool big = box > (size_t)kClipWaveBox;
        const u64 draw = 2 * (u64)id + (u64)fan;
        if (have && !big)
            clip_walk<NS>(t, rcp_exact((float)t.area2), draw, keys, W, a.pattern, px0, px1, py0, py1, box <= (size_t)kMsaaSmallBox, 0, 1);
        // the wave's big fan triangles, one after the other: every lane takes a share of each row's open columns
        u64 m = __ballot(have && big);
        while (m) {
            const int src = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            TriSetup tb = t;
            shfl_tri(tb, src);
            const u64 db = ((u64)__shfl((uint32_t)(draw >> 32), src) << 32) | (u64)__shfl((uint32_t)draw, src);
            const int bx0 = max(0, floordiv_subpix(tb.minX) - 1), bx1 = min(W - 1, floordiv_subpix(tb.maxX) + 1);
            const int by0 = max(0, floordiv_subpix(tb.minY) - 1), by1 = min(H - 1, floordiv_subpix(tb.maxY) + 1);
            clip_walk<NS>(tb, rcp_exact((float)tb.area2), db, keys, W, a.pattern, bx0, bx1, by0, by1, false, lane, warpSize);
        }
    }
}

// grid: (up to kClipBlocks, eye, frame slot), source triangles in a grid-stride loop.  flags: nullptr = every eye.
template <int NS>
__global__ void __launch_bounds__(kMsaaTPB) k_clip_raster(const MsaaArgs a, const uint32_t* flags)
{
    const int W = a.W, H = a.H;
    const int eye = (int)blockIdx.y, slot = (int)blockIdx.z, fr = a.frame0 + slot;
    if (flags && flags[2 * slot + eye] == 0u) return;            // (uniform per block)
    const uint32_t nitems = 2u * (uint32_t)(W - 1) * (uint32_t)(H - 1);
    const FrameDev& f = a.fp[fr];
    const size_t npx = (size_t)W * (size_t)H;
    unsigned long long* keys = a.keys + ((size_t)slot * 2 + (size_t)eye) * npx * NS;
    for (uint32_t base = blockIdx.x * (uint32_t)kMsaaTPB; base < nitems; base += gridDim.x * (uint32_t)kMsaaTPB)     // (uniform per block)
        clip_raster_item<NS>(a, f, fr, slot, eye, base + threadIdx.x, nitems, keys);
}


// One channel as the oracle rounds it: rint, NaN and negatives -> 0, above 255 -> 255.
__device__ __forceinline__ uint32_t clip_channel(float val)
{
    val = rintf(val);
    if (!(val >= 0.0f)) val = 0.0f;
    if (val > 255.0f) val = 255.0f;
    return (uint32_t)val;
}

// The colour of fan triangle `draw` = 2 d + f at the centre of pixel (x, y) (orc_gl_raster): rint(((q0 c0 + q1 c1) + q2 c2) *
// (1 / izc)), or the plain linear combination where izc <= 0, with the polygon's f32 vertex colours.
__device__ uint32_t clip_shade(const MsaaArgs& a, const FrameDev& f, int fr, int slot, int eye, uint32_t draw, int x, int y)
{
    ClipVert pv[4];
    const int np = clip_source(a, f, fr, slot, eye, draw >> 1, pv);
    const int fan = (int)(draw & 1u);
    TriSetup t;
    if (!fan_triangle(pv, np, fan, a.cull, t)) return a.key_rgb;       // (cannot happen: the triangle posted the key)
    const ClipVert& A = pv[0];
    const ClipVert& B = pv[fan + 1];
    const ClipVert& C = pv[fan + 2];
    i64 c0, c1, c2;
    edge_values(t, x * kSubpix + kSubpix / 2, y * kSubpix + kSubpix / 2, c0, c1, c2);
    const float ra = rcp_exact((float)t.area2);
    const float l0 = (float)c0 * ra, l1 = (float)c1 * ra, l2 = (float)c2 * ra;
    const float q0 = l0 * t.iz0, q1 = l1 * t.iz1, q2 = l2 * t.iz2;
    const float izc = (q0 + q1) + q2;
    uint32_t rgb = 0;
    if (izc > 0.0f) {
        const float riz = rcp_exact(izc);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) rgb |= clip_channel(((q0 * A.c[ch] + q1 * B.c[ch]) + q2 * C.c[ch]) * riz) << (8 * ch);
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) rgb |= clip_channel((l0 * A.c[ch] + l1 * B.c[ch]) + l2 * C.c[ch]) << (8 * ch);
    }
    return rgb;
}

template <int NS>
__device__ __forceinline__ void clip_resolve_px(const MsaaArgs& a, int fr, int slot, int eye, size_t o)
{
    const int W = a.W, H = a.H;
    const size_t npx = (size_t)W * (size_t)H;
    bool hole = false;
    if (o < npx) {
        const FrameDev& f = a.fp[fr];
        const int y = (int)(o / (size_t)W), x = (int)(o % (size_t)W);
        unsigned long long* kw = a.keys + ((size_t)slot * 2 + (size_t)eye) * npx * NS + o * NS;
        u64 key[NS];
        uint32_t col[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) key[k] = kw[k];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            col[k] = a.key_rgb;
            if (key[k] == kEmpty64) continue;
            const uint32_t draw = (uint32_t)key[k];
            bool seen = false;
#pragma unroll
            for (int q = 0; q < k; ++q)
                if (!seen && key[q] != kEmpty64 && (uint32_t)key[q] == draw) { col[k] = col[q]; seen = true; }
            if (!seen) col[k] = clip_shade(a, f, fr, slot, eye, draw, x, y);
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) kw[k] = kEmpty64;      // the EMPTY invariant for the next use of the slot
        uint32_t rgb = col[0];
        if (NS == 4) {
            rgb = 0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int sh = 8 * ch;
                rgb |= resolve_channel((col[0] >> sh) & 0xFFu, (col[NS > 1 ? 1 : 0] >> sh) & 0xFFu, (col[NS > 2 ? 2 : 0] >> sh) & 0xFFu,
                                       (col[NS > 3 ? 3 : 0] >> sh) & 0xFFu, a.resolve) << sh;
            }
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

// grid: (up to kClipBlocks, eye, frame slot), pixels in a grid-stride loop.  flags: nullptr = every eye.
template <int NS>
__global__ void __launch_bounds__(kMsaaTPB) k_clip_resolve(const MsaaArgs a, const uint32_t* flags)
{
    const int W = a.W, H = a.H;
    const int eye = (int)blockIdx.y, slot = (int)blockIdx.z, fr = a.frame0 + slot;
    if (flags && flags[2 * slot + eye] == 0u) return;            // (uniform per block)
    const size_t npx = (size_t)W * (size_t)H;
    for (size_t base = (size_t)blockIdx.x * kMsaaTPB; base < npx; base += (size_t)gridDim.x * kMsaaTPB)      // (uniform per block)
        clip_resolve_px<NS>(a, fr, slot, eye, base + threadIdx.x);
}


}  // namespace

hipError_t launch_near_clip_render(const MsaaArgs& a, int n, int samples, uint32_t* flags, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    const size_t npx = (size_t)a.W * (size_t)a.H;
    const size_t items = 2 * (size_t)(a.W - 1) * (size_t)(a.H - 1);
    const unsigned bt = (unsigned)std::min<size_t>((items + kMsaaTPB - 1) / kMsaaTPB, kClipBlocks);
    const unsigned bp = (unsigned)std::min<size_t>((npx + kMsaaTPB - 1) / kMsaaTPB, kClipBlocks);
    const dim3 gt(bt, 2, (unsigned)n), gp(bp, 2, (unsigned)n);
    if (flags) hipLaunchKernelGGL(k_clip_detect, dim3(bp, 1, (unsigned)n), dim3(kMsaaTPB), 0, s, a, flags);
    if (samples == 4) {
        hipLaunchKernelGGL(k_clip_raster<4>, gt, dim3(kMsaaTPB), 0, s, a, (const uint32_t*)flags);
        hipLaunchKernelGGL(k_clip_resolve<4>, gp, dim3(kMsaaTPB), 0, s, a, (const uint32_t*)flags);
    } else {
        hipLaunchKernelGGL(k_clip_raster<1>, gt, dim3(kMsaaTPB), 0, s, a, (const uint32_t*)flags);
        hipLaunchKernelGGL(k_clip_resolve<1>, gp, dim3(kMsaaTPB), 0, s, a, (const uint32_t*)flags);
    }
    return hipGetLastError();
}

}  // namespace MDVT_GRID
}  // namespace mdvt
