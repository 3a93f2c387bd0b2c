// mdvt_general_paths.hip -- what the two GENERAL paths (pose / convergence / K != Krender: global 64-bit z keys instead of a row's
// LDS) share, and the points path whole: k_points_splat_general, the edge points of either mode into the global edge keys
// (k_edge_vertices_list, k_edge_points_splat_list, k_edge_points_splat4, k_edge_keys_reset), k_edge_point_pixels and the resolve of
// both paths, k_resolve_general.  The general mesh path's rasteriser is mdvt_mesh_general.hip.  Each launcher sits below its kernels;
// launch_points_general and launch_mesh_general, the two paths as launch_render (mdvt_render_dispatch.hip) calls them, are at the end.
//
// Compiled with -ffp-contract=off: see the arithmetic decree in mdvt_device.h / DESIGN.md.
#include "mdvt_device.h"

#include <stdlib.h>

namespace mdvt {
namespace MDVT_GRID {      // one copy per sub-pixel grid (mdvt_internal.h)
// =================================================================================================
// POINT MODE, general (pose / convergence / K != Krender): global 64-bit z keys
// =================================================================================================
//   key = f32 bits of Z' << 32 | i << 16 | j      (Z' > 0, so the bit pattern orders like the value)

// An edge point's key into the general paths' edge-key plane.  Whoever finds the word EMPTY also lists it (segment of the
// point's source row: at most one word per vertex and eye, so 2 W entries hold them all): the resolve pass then reads the
// edge keys only where the render left a hole, and k_edge_keys_reset empties exactly the written words -- instead of the
// resolve rewriting the whole plane (8 B/px per eye) for the ~3 % of the words that were touched.
// The lanes of a wave that reach this together (`on`: this lane has a key to post) list their first writes with ONE atomic per
// source row among them (r05): neighbouring lanes work on neighbouring vertices of one source row, and a returning atomic per lane on
// that row's counter -- ~60 of them per row from all over the chip -- was most of the splat's time (96 us per 8 frames for 428
// instructions a vertex).
__device__ __forceinline__ void post_edge_key(const RenderArgs& a, int eye, int fr, int src_row, bool on, size_t pix, u64 key)
{
    u64 old = 0ull;
    if (on) old = atomicMin(&a.ekeys[eye][(size_t)fr * a.ws_stride_px + pix], key);
    const bool first = on && old == kEmpty64;
    const int lane = (int)(threadIdx.x & 63u);
    u64 m = __ballot(first);
    while (m) {                                                     // (uniform over the lanes that are here)
        const int l = __ffsll((long long)m) - 1;
        const int row = __builtin_amdgcn_readlane(src_row, l);
        const bool mine = first && src_row == row;
        const u64 same = __ballot(mine);
        const size_t seg = (size_t)fr * a.H + row;
        uint32_t base = 0;
        if (lane == l) base = atomicAdd(&a.elist_count[seg], (uint32_t)__popcll(same));
        base = (uint32_t)__builtin_amdgcn_readlane((int)base, l);
        if (mine) a.elist[seg * (size_t)(2 * a.W) + base + (uint32_t)__popcll(same & ((1ull << lane) - 1ull))] = ((uint32_t)eye << 31) | (uint32_t)pix;
        m &= ~same;
    }
}

__global__ void __launch_bounds__(64) k_edge_keys_reset(RenderArgs a)
{
    const int fr = blockIdx.y;
    const size_t seg = (size_t)fr * a.H + blockIdx.x;
    const uint32_t n = a.elist_count[seg];
    if (n == 0u) return;
    const uint32_t* list = a.elist + seg * (size_t)(2 * a.W);
    for (uint32_t k = threadIdx.x; k < n; k += 64) {
        const uint32_t e = list[k];
        a.ekeys[e >> 31][(size_t)fr * a.ws_stride_px + (e & 0x7FFFFFFFu)] = kEmpty64;
    }
    if (threadIdx.x == 0) a.elist_count[seg] = 0u;           // (every lane of the one wave has read n)
}

hipError_t launch_edge_keys_reset(const RenderArgs& a, int n, hipStream_t s)
{
    hipLaunchKernelGGL(k_edge_keys_reset, dim3(a.H, n), dim3(64), 0, s, a);
    return hipGetLastError();
}

// (EYES: 2, or 1 for a view render, which splats eye 0 only)
template <int FLAGS, int EYES = 2>
__global__ void __launch_bounds__(256) k_points_splat_general(RenderArgs a)
{
    constexpr bool UNUSED = FLAGS & 2, EDGE = FLAGS & 4, EDGE_ONLY = FLAGS & 8;
    const int W = a.W, H = a.H;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    const int fr = blockIdx.z;
    if (j >= W) return;
    const int f = a.frame0 + fr;
    const FrameDev& fp = a.fp[f];
    const bool un = UNUSED && a.unused[(size_t)fr * a.ws_stride_px + (size_t)i * W + j];
    if (EDGE_ONLY && !un) return;         // mesh mode: only the ~3 % removed vertices are splatted
    const uint8_t* drow = a.depth + (size_t)f * a.depth_stride + (size_t)i * a.depth_pitch;
    const uint32_t code = code16_of(load_px_bytes(drow, j));
    const float z = decode_z(code, fp.mult, fp.scale);
    if (!(z > kNear)) return;
    const float gx = (float)j * fp.sx, gy = (float)i * fp.sy;
    float xc, yc;
    camera_point(fp, gx, gy, z, xc, yc);
    const uint32_t src = ((uint32_t)i << 16) | (uint32_t)j;
    if (!un) {
        if (EDGE_ONLY) return;
#pragma unroll
        for (int eye = 0; eye < EYES; ++eye) {
            const Vert v = vertex_for_eye(fp, eye, gx, gy, z, xc, yc);
            if (!v.ok) continue;
            const int px = point_col(v.u), py = point_row(v.v);
            if (!((uint32_t)px < (uint32_t)W && (uint32_t)py < (uint32_t)H)) continue;
            zkey_post<false>(&a.keys[eye][(size_t)fr * a.ws_stride_px + (size_t)py * W + px], (a.key_parity >> fr) & 1u, __float_as_uint(v.z), src);   // v.z > 0
        }
    } else if (EDGE) {
        EdgePx ep;
        edge_point_pixels(fp, W, H, i, j, fp.sx != 1.0f, z, ep);          // the reference's f64 chain (mdvt_device.h)
#pragma unroll
        for (int eye = 0; eye < 2; ++eye)
            post_edge_key(a, eye, fr, i, ep.ok[eye], (size_t)ep.y[eye] * W + ep.x[eye], ((u64)ep.zkey[eye] << 32) | src);
    }
}

// Mesh mode only splats the removed vertices (~3 % of the grid): the reference's f64 chain, ~10^3 instructions a vertex.  Two launches
// (r05): k_edge_vertices_list turns the 1 B/px plane of `unused` flags into a compact per-frame list of vertices (source row << 16 |
// column; one atomic per workgroup of 16 K pixels), k_edge_points_splat_list runs the chain over the list with every lane busy.
// Until r05 one kernel did both, a workgroup per 8 source rows compacting into LDS: 135 workgroups per 1080p frame, each a chain of
// 15 load / append / barrier steps and two rounds of the chain -- 11.6 us per frame for 3.8 MB, latency all of it.  W % 4 == 0.
// (`valid`: this lane has a vertex; every lane of the wave comes along for post_edge_key's sake)
__device__ __forceinline__ void edge_point_splat_one(const RenderArgs& a, const FrameDev& fp, const uint8_t* dbase, int fr, uint32_t e, bool valid)
{
    const int i = (int)(e >> 16), j = (int)(e & 0xFFFFu);
    EdgePx ep;
    ep.ok[0] = ep.ok[1] = false;
    ep.x[0] = ep.x[1] = ep.y[0] = ep.y[1] = 0;
    ep.zkey[0] = ep.zkey[1] = 0u;
    if (valid) {
        const float z = decode_z(code16_of(load_px_bytes(dbase + (size_t)i * a.depth_pitch, j)), fp.mult, fp.scale);
        if (z > kNear) edge_point_pixels(fp, a.W, a.H, i, j, 1, z, ep);  // the reference's f64 chain (mdvt_device.h)
    }
#pragma unroll
    for (int eye = 0; eye < 2; ++eye)
        post_edge_key(a, eye, fr, i, ep.ok[eye], (size_t)ep.y[eye] * a.W + ep.x[eye], ((u64)ep.zkey[eye] << 32) | e);
}
constexpr int kListTPB = 1024, kListDwords = 4;          // a workgroup of the list pass: 1024 threads x 4 dwords x 4 flags
__global__ void __launch_bounds__(kListTPB) k_edge_vertices_list(RenderArgs a)
{
    __shared__ uint32_t wsum[kListTPB / 64];
    __shared__ uint32_t wbase;
    const int W = a.W, fr = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t ndw = (uint32_t)W * (uint32_t)a.H / 4u;              // (W % 4 == 0: the plane is whole dwords, rows contiguous)
    const uint32_t* flags = (const uint32_t*)(a.unused + (size_t)fr * a.ws_stride_px);
    uint32_t fl[kListDwords], cnt = 0;
#pragma unroll
    for (int k = 0; k < kListDwords; ++k) {
        const uint32_t d = (blockIdx.x * kListDwords + k) * kListTPB + tid;
        fl[k] = d < ndw ? flags[d] : 0u;
        cnt += ((fl[k] & 0xFFu) != 0u) + ((fl[k] & 0xFF00u) != 0u) + ((fl[k] & 0xFF0000u) != 0u) + ((fl[k] >> 24) != 0u);
    }
    uint32_t inc = cnt;                                                   // inclusive sums along the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)inc, off); if (lane >= off) inc += v; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int k = 0; k < kListTPB / 64; ++k) { const uint32_t v = wsum[k]; wsum[k] = run; run += v; }
        wbase = run ? atomicAdd(&a.vlist_count[fr], run) : 0u;
    }
    __syncthreads();
    if (!cnt) return;
    uint32_t* out = a.vlist + (size_t)fr * a.ws_stride_px + wbase + wsum[wave] + (inc - cnt);
#pragma unroll
    for (int k = 0; k < kListDwords; ++k) {
        if (!fl[k]) continue;
        const uint32_t o = ((blockIdx.x * kListDwords + k) * kListTPB + tid) * 4u;
        const uint32_t i = o / (uint32_t)W, j = o - i * (uint32_t)W;      // (the dword's four pixels share a row)
#pragma unroll
        for (int q = 0; q < 4; ++q) if ((fl[k] >> (8 * q)) & 0xFFu) *out++ = (i << 16) | (j + (uint32_t)q);
    }
}
__global__ void __launch_bounds__(256) k_edge_points_splat_list(RenderArgs a)
{
    const int fr = blockIdx.y, f = a.frame0 + fr;
    const FrameDev& fp = a.fp[f];
    const uint8_t* dbase = a.depth + (size_t)f * a.depth_stride;
    const uint32_t total = a.vlist_count[fr];
    const uint32_t* list = a.vlist + (size_t)fr * a.ws_stride_px;
    for (uint32_t k0 = blockIdx.x * 256u; k0 < total; k0 += gridDim.x * 256u) {          // (workgroup uniform)
        const uint32_t k = k0 + threadIdx.x;
        edge_point_splat_one(a, fp, dbase, fr, k < total ? list[k] : 0u, k < total);
    }
}

// The one-kernel form (until r05 the only one; kept for launches under a POSE, where the list form measures 4.6 % slower -- 1080p x 32
// with a pose and edge removal 13.0 -> 12.4 k frames/s, C4 mesh with edge removal 3.06 -> 2.92 k -- while convergence-only launches
// gain from it: product default 12.5 -> 12.9 k, a single frame 163 -> 143 us).  A workgroup scans kSplatRows source rows of the flag
// plane, compacts the flagged vertices of all of them into one list in LDS and runs the chain over it 256 vertices at a time.
constexpr int kSplatRows = 8;
__global__ void __launch_bounds__(256) k_edge_points_splat4(RenderArgs a)
{
    const int W = a.W, H = a.H;
    const int fr = blockIdx.y, tid = threadIdx.x;
    const int i0 = blockIdx.x * kSplatRows, rows = min(kSplatRows, H - i0);
    __shared__ uint32_t list[1024 + 256];             // source row << 16 | column: a step adds at most 1024, fewer than 256 stay behind
    __shared__ uint32_t cnt;
    if (tid == 0) cnt = 0u;
    __syncthreads();
    const int f = a.frame0 + fr;
    const FrameDev& fp = a.fp[f];
    const uint8_t* dbase = a.depth + (size_t)f * a.depth_stride;
    const uint8_t* ubase = a.unused + (size_t)fr * a.ws_stride_px + (size_t)i0 * W;
    const int per_row = W / 4, total = rows * per_row;
    for (int g0 = 0; g0 < total; g0 += 256) {         // (workgroup uniform)
        const int g = g0 + tid;
        uint32_t flags = 0;
        if (g < total) flags = *(const uint32_t*)(ubase + (size_t)g * 4);          // (rows are contiguous: W % 4 == 0)
        if (flags) {
            const uint32_t b0 = (flags & 0xFFu) != 0u, b1 = (flags & 0xFF00u) != 0u, b2 = (flags & 0xFF0000u) != 0u, b3 = (flags >> 24) != 0u;
            uint32_t pos = atomicAdd(&cnt, b0 + b1 + b2 + b3);
            const uint32_t r = (uint32_t)(g / per_row), col = (uint32_t)(g - (int)r * per_row) * 4u;
            const uint32_t base = (((uint32_t)i0 + r) << 16) | col;
            if (b0) list[pos++] = base;
            if (b1) list[pos++] = base + 1u;
            if (b2) list[pos++] = base + 2u;
            if (b3) list[pos++] = base + 3u;
        }
        __syncthreads();
        uint32_t n = cnt;
        while (n >= 256u) {
            n -= 256u;
            edge_point_splat_one(a, fp, dbase, fr, list[n + tid], true);
        }
        __syncthreads();
        if (tid == 0) cnt = n;
        __syncthreads();
    }
    if (cnt) edge_point_splat_one(a, fp, dbase, fr, (uint32_t)tid < cnt ? list[tid] : 0u, (uint32_t)tid < cnt);      // (uniform: cnt is the workgroup's)
}

// mesh mode: the vertices of removed triangles into the global edge keys (sr:589-606)
hipError_t launch_edge_points_splat(const RenderArgs& a, int n, bool as_list, bool counters_zeroed, hipStream_t s)
{
    if (a.W % 4 == 0 && a.vlist && as_list) {
        if (!counters_zeroed) {                              // (the general path's k_mesh_queue_reset has done it on its way)
            hipError_t e = hipMemsetAsync(a.vlist_count, 0, (size_t)n * sizeof(uint32_t), s);
            if (e != hipSuccess) return e;
        }
        const uint32_t ndw = (uint32_t)a.W * (uint32_t)a.H / 4u, per = (uint32_t)(kListTPB * kListDwords);
        hipLaunchKernelGGL(k_edge_vertices_list, dim3((ndw + per - 1) / per, n), dim3(kListTPB), 0, s, a);
        hipLaunchKernelGGL(k_edge_points_splat_list, dim3(256, n), dim3(256), 0, s, a);
    } else if (a.W % 4 == 0) {
        const dim3 grid_s((a.H + kSplatRows - 1) / kSplatRows, n);
        hipLaunchKernelGGL(k_edge_points_splat4, grid_s, dim3(256), 0, s, a);
    } else {
        const dim3 grid_s((a.W + 255) / 256, a.H, n);
        hipLaunchKernelGGL((k_points_splat_general<14>), grid_s, dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

// mdvt_edge_point_pixels: the pixel the edge point of EVERY vertex of one frame lands on, both eyes (INT32_MIN twice: outside
// the frame, or depth code 0).  how = 0: the chain, as the global-key kernels and k_edge_rows_exact take it; how = 1: as the
// LDS row kernels of a pure-shift frame take it -- column from the f32 estimate unless it lies within the guard of a tie
// (edge_col_pure), row = the source row, the scanlines of edge_row_deferred by the chain.
__global__ void __launch_bounds__(256) k_edge_point_pixels(const uint8_t* depth, size_t pitch, const FrameDev* fpp, int W, int H,
                                                           int of_by_one, int how, int32_t* out)
{
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= W) return;
    const FrameDev& fp = fpp[0];
    const float z = decode_z(code16_of(load_px_bytes(depth + (size_t)i * pitch, j)), fp.mult, fp.scale);
    int32_t* o = out + 4 * ((size_t)i * W + j);
    EdgePx ep;
    ep.ok[0] = ep.ok[1] = false;
    if (how == 0 || edge_row_deferred(fp, i)) edge_point_pixels(fp, W, H, i, j, of_by_one, z, ep);
    else if (z > kNear) {
        const float guard = edge_col_guard(W), gx = (float)j * fp.sx, d = fp.dl / z;
#pragma unroll
        for (int eye = 0; eye < 2; ++eye) {
            ep.x[eye] = edge_col_pure(fp, eye, gx, z, d, W, guard);
            ep.y[eye] = i;
            ep.ok[eye] = ep.x[eye] >= 0;
        }
    }
#pragma unroll
    for (int eye = 0; eye < 2; ++eye) {
        o[2 * eye] = ep.ok[eye] ? ep.x[eye] : INT32_MIN;
        o[2 * eye + 1] = ep.ok[eye] ? ep.y[eye] : INT32_MIN;
    }
}

hipError_t launch_edge_point_pixels(const uint8_t* depth, size_t pitch, const FrameDev* fp, int W, int H, int of_by_one, int how,
                                    int32_t* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_edge_point_pixels, dim3((W + 255) / 256, H), dim3(256), 0, s, depth, pitch, fp, W, H, of_by_one, how, out);
    return hipGetLastError();
}

// Resolve of both general paths: PX pixels per thread, coalesced key reads; the z keys need no clearing pass (parity
// scheme, mdvt_device.h: only the uncovered words are rewritten; the edge keys: k_edge_keys_reset), colour from the key word (mesh: colour
// keys) or gathered from the source frame by the winning source index (points).
// (EYES = 1, a view render: eye 0 only; a hole keeps the key colour (3dv:254 writes the render as it comes), the mask is optional and
//  a.hole_counts, where given, is one zeroed word per frame of the batch that every wave adds its holes to)
template <int PX, int FLAGS, bool MESH, int EYES = 2>
__global__ void __launch_bounds__(256) k_resolve_general(RenderArgs a)
{
    constexpr bool ZOUT = FLAGS & 1, EDGE = FLAGS & 4, SEED = FLAGS & 8;
    const int W = a.W;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int fr = EYES == 2 ? blockIdx.z >> 1 : blockIdx.z, eye = EYES == 2 ? blockIdx.z & 1 : 0;
    if (g >= W / PX) return;
    if (MDVT_DEBUG_SKIP(a) & 512) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // (r05 diagnosis, tuning build)
    const int f = a.frame0 + fr;
    const uint8_t* cbase = a.color + (size_t)f * a.color_stride;
    u64* krow = a.keys[eye] + (size_t)fr * a.ws_stride_px + (size_t)y * W + (size_t)g * PX;
    u64* erow = EDGE ? a.ekeys[eye] + (size_t)fr * a.ws_stride_px + (size_t)y * W + (size_t)g * PX : nullptr;
    const uint32_t parity = (a.key_parity >> fr) & 1u;
    u64 key[PX];
#pragma unroll
    for (int q = 0; q < PX; ++q) key[q] = krow[q];
#pragma unroll
    for (int q = 0; q < PX; ++q)                               // only what this use left uncovered needs the next use's empty value
        if (!zkey_covered(key[q], parity)) krow[q] = zkey_empty(parity ^ 1u);
    uint32_t opx[PX], om[PX], spx[PX];
    float oz[PX];
    const u64* crow = MESH ? a.cbuf[eye] + (size_t)fr * a.ws_stride_px + (size_t)y * W + (size_t)g * PX : nullptr;
#pragma unroll
    for (int q = 0; q < PX; ++q) {
        const bool covered = zkey_covered(key[q], parity);
        uint32_t rgb = 0;
        float zval = 0.0f;
        uint32_t kdepth = 0, ktie = 0;
        if (covered) {
            if (MESH) zkey_decode<true>(key[q], parity, kdepth, ktie); else zkey_decode<false>(key[q], parity, kdepth, ktie);
            if (MESH) {
                // the word carries the nearest fragment's colour -- unless the pixel was marked as an exact depth tie between colours:
                // then the rasteriser's second pass left draw id << 32 | colour of the first-drawn fragment at that depth in the side word
                if (ZOUT) zval = 1.0f / __uint_as_float(kdepth);
                rgb = ktie & 0xFFFFFFu;
                if (!(ktie & kNoTie)) rgb = (uint32_t)crow[q] & 0xFFFFFFu;
            } else {
                const uint32_t src = ktie;
                rgb = load_px_bytes(cbase + (size_t)(src >> 16) * a.color_pitch, (int)(src & 0xFFFFu));
                if (ZOUT) zval = __uint_as_float(kdepth);
            }
        }
        const bool hole = !covered || rgb == a.key_rgb;
        uint32_t out = hole ? (EYES == 2 ? 0u : a.key_rgb) : rgb;
        uint32_t esrc = ~0u;
        if (EDGE && hole) {          // an edge point only matters where the render left a hole (sr:776): ~3 % of the pixels
            const u64 ek = erow[q];
            if (ek != kEmpty64) {
                esrc = (uint32_t)ek;
                if (a.edge_paint) out = load_px_bytes(cbase + (size_t)(esrc >> 16) * a.color_pitch, (int)(esrc & 0xFFFFu));
            }
        }
        opx[q] = out;
        om[q] = hole ? 255u : 0u;
        oz[q] = zval;
        if (SEED && a.seed[eye]) spx[q] = seed_pixel(a, a.fp[f], f, eye, g * PX + q, y, hole, esrc, MESH ? 1 : 0);
    }
    if (SEED && a.seed[eye]) RowIO<PX>::store_rgb(a.seed[eye] + (size_t)f * a.seed_stride + (size_t)y * a.seed_pitch, g, spx);
    RowIO<PX>::store_rgb(a.rgb[eye] + (size_t)f * a.rgb_stride + (size_t)y * a.rgb_pitch, g, opx);
    if (EYES == 2 || a.mask[eye]) RowIO<PX>::store_mask(a.mask[eye] + (size_t)f * a.mask_stride + (size_t)y * a.mask_pitch, g, om);
    if (EYES == 1 && a.hole_counts) {
        uint32_t cnt = 0;
#pragma unroll
        for (int q = 0; q < PX; ++q) cnt += (uint32_t)__popcll(__ballot(om[q] != 0u));
        if ((threadIdx.x & 63u) == 0u && cnt) atomicAdd(&a.hole_counts[f], cnt);      // (lane 0 holds the wave's smallest g: active if any lane is)
    }
    if (ZOUT && a.zout[eye])
        RowIO<PX>::store_z((float*)((uint8_t*)a.zout[eye] + (size_t)f * a.zout_stride + (size_t)y * a.zout_pitch), g, oz);
}

template <bool MESH>
static hipError_t launch_resolve_general(const RenderPlan& plan, const RenderArgs& a, hipStream_t s)
{
    const bool zout = a.zout[0] || a.zout[1];
    const bool edge = plan.remove_edges && plan.edge_points;
    const int flags = (zout ? 1 : 0) | (edge ? 4 : 0) | (a.seed[0] ? 8 : 0);
    const int px = plan.vec4 ? 4 : 1;
    if (plan.eyes == 1) {            // a view render: one image per frame, no edge points, no seed
        const dim3 grid1((a.W / px + 255) / 256, a.H, plan.n);
        if (edge || a.seed[0]) return hipErrorInvalidValue;
        if (zout) { if (px == 4) hipLaunchKernelGGL((k_resolve_general<4, 1, MESH, 1>), grid1, dim3(256), 0, s, a); else hipLaunchKernelGGL((k_resolve_general<1, 1, MESH, 1>), grid1, dim3(256), 0, s, a); }
        else { if (px == 4) hipLaunchKernelGGL((k_resolve_general<4, 0, MESH, 1>), grid1, dim3(256), 0, s, a); else hipLaunchKernelGGL((k_resolve_general<1, 0, MESH, 1>), grid1, dim3(256), 0, s, a); }
        return hipGetLastError();
    }
    const dim3 grid((a.W / px + 255) / 256, a.H, plan.n * 2), block(256);
#define MDVT_CASE(F)                                                                                  \
    case F:                                                                                           \
        if (px == 4) hipLaunchKernelGGL((k_resolve_general<4, F, MESH>), grid, block, 0, s, a);       \
        else hipLaunchKernelGGL((k_resolve_general<1, F, MESH>), grid, block, 0, s, a);               \
        break;
    switch (flags) {
        MDVT_CASE(0) MDVT_CASE(1) MDVT_CASE(4) MDVT_CASE(5) MDVT_CASE(8) MDVT_CASE(9) MDVT_CASE(12) MDVT_CASE(13)
    }
#undef MDVT_CASE
    if (edge) return launch_edge_keys_reset(a, plan.n, s);
    return hipGetLastError();
}

// The global key buffers are EMPTY on entry: the host clears them when they are (re)allocated and every
// resolve pass leaves them EMPTY again.
hipError_t launch_points_general(const RenderPlan& plan, const RenderArgs& a, hipStream_t s)
{
    const bool edge = plan.remove_edges && plan.edge_points;
    hipError_t e;
    const dim3 block(256);
    const dim3 grid_s((a.W + 255) / 256, a.H, plan.n);
    const int sflags = (plan.remove_edges ? 2 : 0) | (edge ? 4 : 0);
    if (plan.eyes == 1) {
        if (edge) return hipErrorInvalidValue;
        if (plan.remove_edges) hipLaunchKernelGGL((k_points_splat_general<2, 1>), grid_s, block, 0, s, a);
        else hipLaunchKernelGGL((k_points_splat_general<0, 1>), grid_s, block, 0, s, a);
    } else
    switch (sflags) {
        case 0: hipLaunchKernelGGL((k_points_splat_general<0>), grid_s, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((k_points_splat_general<2>), grid_s, block, 0, s, a); break;
        default: hipLaunchKernelGGL((k_points_splat_general<6>), grid_s, block, 0, s, a); break;
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (plan.after_vertices && (e = hipEventRecord(plan.after_vertices, s)) != hipSuccess) return e;     // (banks: the next set may start)
    return launch_resolve_general<false>(plan, a, s);
}

hipError_t launch_mesh_general(const RenderPlan& plan, const RenderArgs& a_in, hipStream_t s)
{
    RenderArgs a = a_in;
    if (const char* e = tuning_env(TUNE_DEBUG_SKIP)) a.debug_skip = atoi(e);
    const bool edge = plan.remove_edges && plan.edge_points;
    hipError_t e;
    if ((e = launch_mesh_raster_general(plan, a, s)) != hipSuccess) return e;
    if (edge && (e = launch_edge_points_splat(a, plan.n, plan.conv_raster != 0, true, s)) != hipSuccess) return e;
    return launch_resolve_general<true>(plan, a, s);
}

}  // namespace MDVT_GRID
}  // namespace mdvt
