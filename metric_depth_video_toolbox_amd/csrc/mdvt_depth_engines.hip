// mdvt_depth_engines.hip -- the non-model work of the reference's per-frame depth engines and of its PromptDA upscaler
// (include/mdvt_depth_engines.h): packed video frames to a model's planar input (mdvt_model_frames), a coded depth video to PromptDA's
// low-resolution prompt (mdvt_depth_prompt) and UniK3D's focal estimate from its point map (mdvt_focal_from_points).
//
// The unit is compiled with -ffp-contract=off, IEEE division and without fast-math (Makefile): every `*`, `+`, `-` and `/` below is
// one IEEE operation, rounded before the next.  Shared with other units: mdvt_depth_code.h (the four-pixel frame quad_of, and for the
// prompt the float32 gather quad_gather over this unit's CodeSource), mdvt_adapter_resize.h (the u8 resize), mdvt_pairwise.h (NumPy's
// order of summation) and mdvt_ordered_select.h (the scan of the unit counts and the mean from the chunk sums, as in
// mdvt_convergence.hip).
//
// k_model_frames, k_depth_prompt: a thread per four output pixels of a row, a frame per blockIdx.y.  Packed
// 3-byte pixels are read as 12 bytes per lane where nothing is resized and the source is aligned to 4: the three dwords are adjacent, so
// the lanes of a wave read one run of 768 bytes and every byte of a cache line is used; the planar stores are 4 or 16 bytes per lane,
// neighbouring lanes neighbouring addresses.  Resized pixels gather their taps byte by byte: the taps of neighbouring pixels are
// neighbours or the same, and the caches serve them.  A value's arithmetic does not depend on which loads and stores it takes.
//
// The focal estimate per launch set (count, compact and reduce are this unit's own: both lists of a frame from one walk, float values):
//   k_focal_count    one wave per unit of 2048 points: both selections as ballots, the unit's two counts
//   k_focal_scan     one wave per list (a frame's ex, or its ey): exclusive scan of the unit counts, the list's count
//   k_focal_compact  one wave per unit: the points again, ex and ey of the selected ones in row-major order to their places
//   k_focal_reduce   one workgroup per chunk of 8192 values of a list: the chunk in LDS (a padding dword per 128 values, so that the
//                    leaves' threads read different banks), walked in the general shape of mdvt_pairwise.h -- a full chunk is that
//                    shape's balanced tree over 64 leaves of 128 values
//   k_focal_mean     one wave per list: the chunk sums in order, the division, the 0 of an empty selection, the count
// Every sum has a fixed shape: no floating-point atomics, no dependence on the launch geometry.
#include "mdvt_internal.h"
#include "mdvt_adapter_resize.h"
#include "mdvt_depth_code.h"
#include "mdvt_ordered_select.h"

namespace mdvt {
namespace {

using depth_code::store_plane;
using depth_code::Quad;
using depth_code::quad_of;
using depth_code::quad_gather;
using pairwise::kChunk;

// ---- mdvt_model_frames ---------------------------------------------------------------------------------------------------------

template <bool AS_FLOAT>
__global__ void __launch_bounds__(256) k_model_frames(ModelFramesArgs a)
{
    Quad q;
    if (!quad_of(a.groups, a.gw, a.rs.out_w, a.frame0, q)) return;
    const uint32_t row = q.row;
    const int x0 = q.x0, nv = q.nv;
    const uint8_t* src = a.src + q.f * a.src_stride;
    const size_t pitch = a.src_pitch;
    uint32_t px[4] = {0u, 0u, 0u, 0u};                              // byte 0 | byte 1 << 8 | byte 2 << 16 as stored
    if (a.rs.mode == 0 && a.src_vec && nv == 4) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(src + (size_t)row * pitch + (size_t)x0 * 3u);
        unpack4(q[0], q[1], q[2], px);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nv) px[k] = adapter_resize_px(a.rs, x0 + k, (int)row, [&](int sx, int sy) { return load_px_bytes(src + (size_t)sy * pitch, sx); });
    }
    uint8_t* out = a.dst + q.f * a.dst_stride + (size_t)row * a.dst_pitch + (size_t)x0 * (AS_FLOAT ? 4u : 1u);
#pragma unroll
    for (int c = 0; c < 3; ++c) {                                   // planes R, G, B
        const int shift = 8 * (a.bgr ? 2 - c : c);
        uint8_t* o = out + (size_t)c * a.dst_plane;
        if (AS_FLOAT) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (float)((px[k] >> shift) & 0xFFu) / 255.0f;
            store_plane(reinterpret_cast<float*>(o), v, nv, a.dst_vec != 0);
        } else if (a.dst_vec && nv == 4) {
            *reinterpret_cast<uint32_t*>(o) = ((px[0] >> shift) & 0xFFu) | (((px[1] >> shift) & 0xFFu) << 8) |
                                              (((px[2] >> shift) & 0xFFu) << 16) | (((px[3] >> shift) & 0xFFu) << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nv) o[k] = (uint8_t)(px[k] >> shift);
        }
    }
}

// ---- mdvt_depth_prompt ---------------------------------------------------------------------------------------------------------

// dfh:21-23 on a pixel as stored: float32(R << 24 | B << 16) * mult.  The conversion is exact (16 significant bits).
__device__ __forceinline__ float decode_px(uint32_t px, int bgr, float mult)
{
    const uint32_t first = px & 0xFFu, third = (px >> 16) & 0xFFu;
    const uint32_t code = bgr ? (third << 24) | (first << 16) : (first << 24) | (third << 16);
    return (float)code * mult;
}

// a coded depth frame as a source of the gather (mdvt_depth_code.h): a pixel decoded, four pixels through the three-dword load
struct CodeSource {
    static constexpr size_t kBytes = 3;
    int bgr; float mult;
    __device__ __forceinline__ float at(const uint8_t* p, int x) const { return decode_px(load_px_bytes(p, x), bgr, mult); }
    __device__ __forceinline__ void four(const uint8_t* p, float (&d)[4]) const
    {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
        uint32_t px[4];
        unpack4(w[0], w[1], w[2], px);
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = decode_px(px[k], bgr, mult);
    }
};

template <bool RESIZE>
__global__ void __launch_bounds__(256) k_depth_prompt(DepthPromptArgs a)
{
    Quad q;
    if (!quad_of(a.groups, a.gw, a.out_w, a.frame0, q)) return;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    quad_gather(d, a.src + q.f * a.src_stride, a.src_pitch, a.src_vec != 0, q, RESIZE, a.ratio_x, a.ratio_y, a.in_w, a.in_h,
                CodeSource{a.bgr, a.mult});
    store_plane(reinterpret_cast<float*>(a.dst + q.f * a.dst_stride + (size_t)q.row * a.dst_pitch) + q.x0, d, q.nv, a.dst_vec != 0);
}

// ---- mdvt_focal_from_points ----------------------------------------------------------------------------------------------------

constexpr float kFocalEps = 1e-6f;                                   // float32(1e-6) (unik3d_video.py:87)

struct FocalPoint { bool sel_x, sel_y; float ex, ey; };

// point p < npx of a frame, in row-major order: both selections and both values (unik3d_video.py:82-95)
__device__ __forceinline__ FocalPoint focal_point(const FocalArgs& a, const uint8_t* frame, uint32_t p)
{
    const uint32_t v = p / a.W, u = p - v * a.W;
    const uint8_t* q = frame + (size_t)v * a.pitch + (size_t)u * a.point_bytes;
    const float X = *reinterpret_cast<const float*>(q);
    const float Y = *reinterpret_cast<const float*>(q + a.chan_bytes);
    const float Z = *reinterpret_cast<const float*>(q + 2 * a.chan_bytes);
    const bool z_ok = fabsf(Z) > kFocalEps;                          // (a NaN compares false)
    FocalPoint o;
    o.sel_x = fabsf(X) > kFocalEps && z_ok;
    o.sel_y = fabsf(Y) > kFocalEps && z_ok;
    o.ex = ((float)u - a.half_w) * (Z / X);
    o.ey = ((float)v - a.half_h) * (Z / Y);
    return o;
}

__global__ void __launch_bounds__(256) k_focal_count(FocalArgs a)
{
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t u = blockIdx.x * 4u + (threadIdx.x >> 6);
    const size_t f = blockIdx.y;
    if (u >= a.nunits) return;
    const uint8_t* frame = a.points + f * a.stride;
    uint32_t cx = 0, cy = 0;
    for (uint32_t g = 0; g < kFocalUnit / 64u; ++g) {
        const uint32_t p = u * kFocalUnit + g * 64u + (uint32_t)lane;
        bool sx = false, sy = false;
        if (p < a.npx) {
            const FocalPoint o = focal_point(a, frame, p);
            sx = o.sel_x; sy = o.sel_y;
        }
        cx += (uint32_t)__popcll(__ballot(sx));
        cy += (uint32_t)__popcll(__ballot(sy));
    }
    if (lane == 0) {
        a.unit_cnt[(2 * f) * a.nunits + u] = cx;
        a.unit_cnt[(2 * f + 1) * a.nunits + u] = cy;
    }
}

__global__ void __launch_bounds__(64) k_focal_scan(FocalArgs a)
{
    const size_t l = blockIdx.x;                                     // the list
    ordered_select::unit_scan(a.unit_cnt + l * a.nunits, a.unit_off + l * a.nunits, a.nunits, a.totals + l);
}

__global__ void __launch_bounds__(256) k_focal_compact(FocalArgs a)
{
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t u = blockIdx.x * 4u + (threadIdx.x >> 6);
    const size_t f = blockIdx.y;
    if (u >= a.nunits) return;
    const uint8_t* frame = a.points + f * a.stride;
    float* dx = a.compact + (2 * f) * a.compact_stride;
    float* dy = a.compact + (2 * f + 1) * a.compact_stride;
    uint32_t ox = a.unit_off[(2 * f) * a.nunits + u];                // < npx, and ox + the unit's count <= npx
    uint32_t oy = a.unit_off[(2 * f + 1) * a.nunits + u];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t g = 0; g < kFocalUnit / 64u; ++g) {
        const uint32_t p = u * kFocalUnit + g * 64u + (uint32_t)lane;
        FocalPoint o{false, false, 0.f, 0.f};
        if (p < a.npx) o = focal_point(a, frame, p);
        const unsigned long long bx = __ballot(o.sel_x), by = __ballot(o.sel_y);
        if (o.sel_x) dx[ox + (uint32_t)__popcll(bx & below)] = o.ex;
        if (o.sel_y) dy[oy + (uint32_t)__popcll(by & below)] = o.ey;
        ox += (uint32_t)__popcll(bx);
        oy += (uint32_t)__popcll(by);
    }
}

constexpr int kFocalReduceThreads = 256;

// the staged chunk: value i at dword i + (i >> 7)
struct StagedValues {
    const float* s;
    __device__ __forceinline__ float operator()(int i) const { return s[i + (i >> 7)]; }
};

__global__ void __launch_bounds__(kFocalReduceThreads) k_focal_reduce(FocalArgs a)
{
    __shared__ float s_val[kChunk + kChunk / 128];
    __shared__ pairwise::Shape s_shape;
    const int tid = (int)threadIdx.x;
    const uint32_t c = blockIdx.x;
    const size_t l = blockIdx.y;
    const uint32_t total = a.totals[l];
    const uint32_t first = c * (uint32_t)kChunk;
    if (first >= total) return;                                      // (uniform: the whole workgroup leaves)
    const int n = (int)(total - first < (uint32_t)kChunk ? total - first : (uint32_t)kChunk);
    const float* src = a.compact + l * a.compact_stride + first;
    for (int i = tid; i < n; i += kFocalReduceThreads) s_val[i + (i >> 7)] = src[i];
    if (tid == 0) pairwise::shape_list(s_shape, n);
    __syncthreads();
    pairwise::shape_leaves(s_shape, StagedValues{s_val}, tid);
    __syncthreads();
    if (tid == 0) a.sums[l * a.nchunks + c] = pairwise::shape_join(s_shape);
}

__global__ void __launch_bounds__(64) k_focal_mean(FocalArgs a)
{
    const size_t l = blockIdx.x;                                     // the list
    const uint32_t total = a.totals[l];
    const float mean = ordered_select::ordered_mean(a.sums + l * a.nchunks, total, 0.0f);      // unik3d_video.py:98-99
    if (threadIdx.x == 0) {
        a.focal[l] = mean;
        if (a.counts) a.counts[l] = total;
    }
}

}  // namespace

hipError_t launch_model_frames(const ModelFramesArgs& a, int n_frames, hipStream_t s)
{
    const dim3 grid((a.groups + 255u) / 256u, (unsigned)n_frames);
    if (a.as_float) hipLaunchKernelGGL(k_model_frames<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_model_frames<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_depth_prompt(const DepthPromptArgs& a, int n_frames, hipStream_t s)
{
    const dim3 grid((a.groups + 255u) / 256u, (unsigned)n_frames);
    if (a.resize) hipLaunchKernelGGL(k_depth_prompt<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_depth_prompt<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_focal_from_points(const FocalArgs& a, hipStream_t s)
{
    const dim3 units((a.nunits + 3u) / 4u, (unsigned)a.n_frames);
    const unsigned lists = 2u * (unsigned)a.n_frames;
    hipLaunchKernelGGL(k_focal_count, units, dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_focal_scan, dim3(lists), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_focal_compact, units, dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_focal_reduce, dim3(a.nchunks, lists), dim3(kFocalReduceThreads), 0, s, a);
    hipLaunchKernelGGL(k_focal_mean, dim3(lists), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdvt
