// mdvt_geometry.hip -- the geometry export (include/mdvt_geometry.h): every vertex of a frame, the triangles the 89-degree filter
// keeps in the reference's draw order, the used vertices in index order (cmf:692-749), and the grey depth of cmf:752-760.
// Depends neither on the sub-pixel grid nor on a tuning hook: compiled once and linked into both libraries.
//
// The arithmetic.  The vertex is vertex_f64 (mdvt_device.h), the filter's verdict edge_filter_cell (mdvt_edge_filter.h) -- the
// functions the renders use, not a copy --, the pose Open3D's point transform as mdvt_view.hip evaluates it.  One IEEE operation per
// node, no contraction (Makefile).
//
// The compaction.  A frame has two lists: its 2 ncell triangles in draw order (all tri1 row-major, then all tri2) and its N vertices.
// An item is kept by a predicate that reads nothing but the filter's flags: a triangle if its flag is clear, a vertex if one of the
// (up to) six triangles around it is kept -- gathered, not scattered, so no store order is involved.  Per launch set:
//   k_geom_vertices  one thread per vertex: the posed vertex into `vertices` (where given)
//   k_geom_flags     one thread per cell: both triangles' verdicts as bytes [2 ncell] (remove_edges only)
//   k_geom_count     one workgroup per kGeomBlock items of a list: the kept ones -- a ballot and a popcount per wave, the four waves
//                    joined in LDS -- into totals[frame][workgroup]
//   k_geom_scan      one workgroup per frame and list: totals -> the kept items before each workgroup (kGeomScan totals a step, the
//                    running sum carried by the same workgroup from step to step), the list's length into counts
//   k_geom_scatter   the count's predicate again; an item's place is its workgroup's offset + the kept items of the waves before its
//                    own + the kept lanes below it: triangles, used_index, points and point_rgb are written there
// Separate launches at each seam: no workgroup waits for another, and there is no atomic.  Places depend on the predicate alone.
#include "mdvt_edge_filter.h"

namespace mdvt {
namespace {

// cmf:646-652 (decode 0: the high byte is (R + G) >> 1, ONE correctly rounded division by f32(255^4 / max_depth)) or dfh:21-23 (decode 1:
// decode_z's multiply); then * f32(depth_scale)
__device__ __forceinline__ float geom_z(uint32_t px, int decode, float mult, float scale)
{
    if (decode) return decode_z(code16_of(px), mult, scale);
    const uint32_t hi = ((px & 0xFFu) + ((px >> 8) & 0xFFu)) >> 1;
    const float d = (float)(((hi << 8) | (px >> 16)) << 16) / mult;
    return d * scale;
}

__device__ __forceinline__ float geom_z_at(const GeometryArgs& a, const FrameDev& f, const uint8_t* frame, int i, int j)
{
    return geom_z(load_px_bytes(frame + (size_t)i * a.depth_pitch, j), a.decode, f.mult, f.scale);
}

// vertex v of a frame: dmt:1112-1133 with of_by_one, then cmf:694-695
__device__ __forceinline__ void geom_vertex(const GeometryArgs& a, const FrameDev& f, const uint8_t* frame, uint32_t v, double (&p)[3])
{
    const uint32_t i = v / (uint32_t)a.W, j = v - i * (uint32_t)a.W;
    vertex_f64(f, (int)i, (int)j, 1, geom_z_at(a, f, frame, (int)i, (int)j), p);
    if (f.has_T) {
        const double* T = f.Td;
        double hh[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) hh[r] = ((T[4 * r] * p[0] + T[4 * r + 1] * p[1]) + T[4 * r + 2] * p[2]) + T[4 * r + 3] * 1.0;
        if (hh[3] != 1.0) { hh[0] = hh[0] / hh[3]; hh[1] = hh[1] / hh[3]; hh[2] = hh[2] / hh[3]; }     // (x / 1.0 == x)
        p[0] = hh[0]; p[1] = hh[1]; p[2] = hh[2];
    }
}

__global__ void __launch_bounds__(256) k_geom_vertices(GeometryArgs a)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= a.npx) return;
    const size_t f = (size_t)a.frame0 + blockIdx.y;
    double p[3];
    geom_vertex(a, a.fp[f], a.depth + f * a.depth_stride, v, p);
    double* o = (double*)((uint8_t*)a.vertices + f * a.vertices_stride) + 3 * (size_t)v;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
}

// k_edge_filter's cell (mdvt_edge_filter.hip) with this call's depth
__global__ void __launch_bounds__(128) k_geom_flags(GeometryArgs a)
{
    const uint32_t c = blockIdx.x * 128u + threadIdx.x;
    if (c >= a.ncell) return;
    const int i = (int)(c / (uint32_t)(a.W - 1)), j = (int)(c - (uint32_t)i * (uint32_t)(a.W - 1));
    const size_t fi = (size_t)a.frame0 + blockIdx.y;
    const FrameDev& f = a.fp[fi];
    const uint8_t* frame = a.depth + fi * a.depth_stride;
    const float zA = geom_z_at(a, f, frame, i, j), zD = geom_z_at(a, f, frame, i, j + 1);
    const float zB = geom_z_at(a, f, frame, i + 1, j), zC = geom_z_at(a, f, frame, i + 1, j + 1);
    const double rfx = f.rKd[0], rfy = f.rKd[1];
    const double x0r = ((double)((float)j * f.sx) - f.Kd[2]) * rfx, x1r = ((double)((float)(j + 1) * f.sx) - f.Kd[2]) * rfx;
    const double y0r = ((double)((float)i * f.sy) - f.Kd[3]) * rfy, y1r = ((double)((float)(i + 1) * f.sy) - f.Kd[3]) * rfy;
    const uint32_t inv = edge_filter_cell(f, i, j, 1, x0r, x1r, y0r, y1r,
                                          edge_filter_prescreen(cell_rays_f32(x0r, x1r, y0r, y1r), zA, zB, zC, zD), zA, zB, zC, zD);
    uint8_t* t = a.flags + (size_t)blockIdx.y * a.flags_stride;
    t[c] = (uint8_t)(inv & 1u);
    t[(size_t)a.ncell + c] = (uint8_t)((inv >> 1) & 1u);
}

// ---- the predicate ---------------------------------------------------------------------------------------------------------------
// flags: the launch-set frame's [2 ncell] bytes, or null (nothing is removed: a frame is at least 2 x 2, every vertex has a triangle)
__device__ __forceinline__ bool tri_kept(const uint8_t* flags, uint32_t t) { return !flags || flags[t] == 0; }

// one of the triangles around vertex (i, j) is kept: tri1 of the cells (i, j) [as A], (i-1, j) [B], (i-1, j-1) [C], tri2 of the cells
// (i, j) [A], (i-1, j-1) [C], (i, j-1) [D]
__device__ __forceinline__ bool vertex_used(const uint8_t* flags, int W, int H, uint32_t ncell, int i, int j)
{
    if (!flags) return true;
    const int cw = W - 1, ch = H - 1;
    bool used = false;
    if (i < ch && j < cw) { const uint32_t c = (uint32_t)i * cw + j; used = flags[c] == 0 || flags[ncell + c] == 0; }
    if (i >= 1 && j < cw) used = used || flags[(uint32_t)(i - 1) * cw + j] == 0;
    if (i >= 1 && j >= 1) { const uint32_t c = (uint32_t)(i - 1) * cw + (j - 1); used = used || flags[c] == 0 || flags[ncell + c] == 0; }
    if (i < ch && j >= 1) used = used || flags[ncell + (uint32_t)i * cw + (j - 1)] == 0;
    return used;
}

// item `item` of workgroup b of a frame's lists: workgroups [0, nbt) take the triangles, [nbt, nbt + nbv) the vertices
__device__ __forceinline__ bool geom_kept(const GeometryArgs& a, const uint8_t* flags, bool tris, uint32_t item)
{
    if (tris) return item < 2u * a.ncell && tri_kept(flags, item);
    if (item >= a.npx) return false;
    const uint32_t i = item / (uint32_t)a.W;
    return vertex_used(flags, a.W, a.H, a.ncell, (int)i, (int)(item - i * (uint32_t)a.W));
}

__global__ void __launch_bounds__(kGeomBlock) k_geom_count(GeometryArgs a)
{
    __shared__ uint32_t s_wave[kGeomBlock / 64];
    const uint32_t b = blockIdx.x, fr = blockIdx.y, tid = threadIdx.x;
    const bool tris = b < a.nbt;
    const uint32_t item = (tris ? b : b - a.nbt) * kGeomBlock + tid;
    const uint8_t* flags = a.flags ? a.flags + (size_t)fr * a.flags_stride : nullptr;
    const unsigned long long m = __ballot(geom_kept(a, flags, tris, item));
    if ((tid & 63u) == 0) s_wave[tid >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (tid == 0) {
        uint32_t n = 0;
#pragma unroll
        for (uint32_t w = 0; w < kGeomBlock / 64; ++w) n += s_wave[w];
        a.totals[(size_t)fr * (a.nbt + a.nbv) + b] = n;
    }
}

// grid (2, frames): list 0 = triangles, list 1 = vertices.  totals -> exclusive offsets, in place; counts[frame] = {U, M}
__global__ void __launch_bounds__(kGeomScan) k_geom_scan(GeometryArgs a)
{
    __shared__ uint32_t s_wave[kGeomScan / 64];
    const uint32_t list = blockIdx.x, fr = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n = list ? a.nbv : a.nbt;
    uint32_t* t = a.totals + (size_t)fr * (a.nbt + a.nbv) + (list ? a.nbt : 0u);
    uint32_t running = 0;
    for (uint32_t base = 0; base < n; base += kGeomScan) {
        const uint32_t k = base + tid;
        const uint32_t v = k < n ? t[k] : 0u;
        uint32_t incl = v;                                               // inclusive scan of the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if ((int)lane >= d) incl += up;
        }
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < kGeomScan / 64; ++w) { before += w < wave ? s_wave[w] : 0u; all += s_wave[w]; }
        if (k < n) t[k] = running + before + (incl - v);
        running += all;
        __syncthreads();                                                 // s_wave is rewritten by the next step
    }
    if (tid == 0) a.counts[2 * ((size_t)a.frame0 + fr) + (list ? 0u : 1u)] = running;
}

__global__ void __launch_bounds__(kGeomBlock) k_geom_scatter(GeometryArgs a)
{
    __shared__ uint32_t s_wave[kGeomBlock / 64];
    const uint32_t b = blockIdx.x, fr = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const bool tris = b < a.nbt;
    if (tris && !a.triangles) return;                                    // (the whole workgroup: a list nobody asked for)
    const uint32_t item = (tris ? b : b - a.nbt) * kGeomBlock + tid;
    const uint8_t* flags = a.flags ? a.flags + (size_t)fr * a.flags_stride : nullptr;
    const bool kept = geom_kept(a, flags, tris, item);
    const unsigned long long m = __ballot(kept);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!kept) return;
    uint32_t at = a.totals[(size_t)fr * (a.nbt + a.nbv) + b] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
#pragma unroll
    for (uint32_t w = 0; w < kGeomBlock / 64; ++w) at += w < wave ? s_wave[w] : 0u;
    const size_t f = (size_t)a.frame0 + fr;
    if (tris) {
        const uint32_t pass = item >= a.ncell ? 1u : 0u, cell = item - pass * a.ncell;
        const uint32_t i = cell / (uint32_t)(a.W - 1), j = cell - i * (uint32_t)(a.W - 1);
        const int32_t idx1 = (int32_t)(i * (uint32_t)a.W + j), idx2 = idx1 + a.W, idx3 = idx2 + 1, idx4 = idx1 + 1;      // dmt:1247-1250
        int32_t* o = (int32_t*)((uint8_t*)a.triangles + f * a.triangles_stride) + 3 * (size_t)at;
        o[0] = idx1;
        o[1] = pass ? idx3 : idx2;                                       // dmt:1252-1253
        o[2] = pass ? idx4 : idx3;
        return;
    }
    if (a.used_index) ((int32_t*)((uint8_t*)a.used_index + f * a.used_stride))[at] = (int32_t)item;
    if (a.points) {
        double p[3];
        geom_vertex(a, a.fp[f], a.depth + f * a.depth_stride, item, p);
        double* o = (double*)((uint8_t*)a.points + f * a.points_stride) + 3 * (size_t)at;
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
    }
    if (a.point_rgb) {
        const uint32_t i = item / (uint32_t)a.W, j = item - i * (uint32_t)a.W;
        const uint32_t px = load_px_bytes(a.color + f * a.color_stride + (size_t)i * a.color_pitch, (int)j);
        uint8_t* o = a.point_rgb + f * a.point_rgb_stride + 3 * (size_t)at;
        o[0] = (uint8_t)px; o[1] = (uint8_t)(px >> 8); o[2] = (uint8_t)(px >> 16);
    }
}

// cmf:752-760: the exporter's depth, one f32 multiply, np.rint, saturated to the type (the header's decree)
__global__ void __launch_bounds__(256) k_depth_grey(const uint8_t* __restrict__ depth, size_t pitch, size_t stride, float divisor, float mult,
                                                    int bits, uint8_t* __restrict__ out, size_t out_pitch, size_t out_stride, int W, uint32_t npx)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= npx) return;
    const uint32_t i = v / (uint32_t)W;
    const int j = (int)(v - i * (uint32_t)W);
    const uint32_t px = load_px_bytes(depth + (size_t)blockIdx.y * stride + (size_t)i * pitch, j);
    const float d = geom_z(px, 0, divisor, 1.0f);                        // (d * 1.0f == d)
    const float r = rintf(d * mult);
    uint8_t* row = out + (size_t)blockIdx.y * out_stride + (size_t)i * out_pitch;
    if (bits == 16) {
        ((uint16_t*)row)[j] = (uint16_t)(uint32_t)fminf(r, 65535.0f);
    } else {
        const uint8_t g = (uint8_t)(uint32_t)fminf(r, 255.0f);
        uint8_t* o = row + 3 * (size_t)j;
        o[0] = g; o[1] = g; o[2] = g;
    }
}

}  // namespace

hipError_t launch_export_geometry(const GeometryArgs& a, hipStream_t s)
{
    const unsigned n = (unsigned)a.n_frames;
    if (a.vertices) hipLaunchKernelGGL(k_geom_vertices, dim3((a.npx + 255u) / 256u, n), dim3(256), 0, s, a);
    if (a.flags) hipLaunchKernelGGL(k_geom_flags, dim3((a.ncell + 127u) / 128u, n), dim3(128), 0, s, a);
    hipLaunchKernelGGL(k_geom_count, dim3(a.nbt + a.nbv, n), dim3(kGeomBlock), 0, s, a);
    hipLaunchKernelGGL(k_geom_scan, dim3(2, n), dim3(kGeomScan), 0, s, a);
    // (the vertex workgroups come last: where only triangles are wanted they are not launched)
    const bool verts = a.used_index || a.points || a.point_rgb;
    if (a.triangles || verts) hipLaunchKernelGGL(k_geom_scatter, dim3(verts ? a.nbt + a.nbv : a.nbt, n), dim3(kGeomBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_depth_grey(const uint8_t* depth, size_t pitch, size_t stride, float divisor, float mult, int bits, void* out,
                             size_t out_pitch, size_t out_stride, int W, int H, int n_frames, hipStream_t s)
{
    constexpr int kFrames = 32768;                                       // frames of one launch (grid.y)
    const unsigned nb = ((unsigned)W * (unsigned)H + 255u) / 256u;
    for (int f0 = 0; f0 < n_frames; f0 += kFrames) {
        const int n = n_frames - f0 < kFrames ? n_frames - f0 : kFrames;
        hipLaunchKernelGGL(k_depth_grey, dim3(nb, (unsigned)n), dim3(256), 0, s, depth + (size_t)f0 * stride, pitch, stride, divisor, mult, bits,
                           (uint8_t*)out + (size_t)f0 * out_stride, out_pitch, out_stride, W, (uint32_t)W * (uint32_t)H);
    }
    return hipGetLastError();
}

}  // namespace mdvt
