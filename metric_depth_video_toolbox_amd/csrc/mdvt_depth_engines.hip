// mdvt_depth_engines.hip -- the non-model work of the reference's per-frame depth engines and of its PromptDA upscaler
// (include/mdvt_depth_engines.h): packed video frames to a model's planar input (mdvt_model_frames), a coded depth video to PromptDA's
// low-resolution prompt (mdvt_depth_prompt) and UniK3D's focal estimate from its point map (mdvt_focal_from_points).
//
// The unit is compiled with -ffp-contract=off, IEEE division and without fast-math (Makefile), like the units it shares
// mdvt_depth_code.h (the float32 resize tables), mdvt_adapter_resize.h (the u8 resize) and mdvt_pairwise.h (NumPy's order of
// summation) with: every `*`, `+`, `-` and `/` below is one IEEE operation, rounded before the next.
//
// k_model_frames, k_depth_prompt: a thread per four output pixels of a row, a frame per blockIdx.y; k_depth_sink is the model.  Packed
// 3-byte pixels are read as 12 bytes per lane where nothing is resized and the source is aligned to 4: the three dwords are adjacent, so
// the lanes of a wave read one run of 768 bytes and every byte of a cache line is used; the planar stores are 4 or 16 bytes per lane,
// neighbouring lanes neighbouring addresses.  Resized pixels gather their taps byte by byte: the taps of neighbouring pixels are
// neighbours or the same, and the caches serve them.  A value's arithmetic does not depend on which loads and stores it takes.
//
// The focal estimate per launch set, modelled on mdvt_convergence.hip:
//   k_focal_count    one wave per unit of 2048 points: both selections as ballots, the unit's two counts
//   k_focal_scan     one wave per list (a frame's ex, or its ey): exclusive scan of the unit counts, the list's count
//   k_focal_compact  one wave per unit: the points again, ex and ey of the selected ones in row-major order to their places
//   k_focal_reduce   one workgroup per chunk of 8192 values of a list: the chunk in LDS (a padding dword per 128 values, so that the
//                    leaves' threads read different banks), walked in the general shape of mdvt_pairwise.h -- a full chunk is that
//                    shape's balanced tree over 64 leaves of 128 values
//   k_focal_mean     one thread per list: the chunk sums in order, the division, the 0 of an empty selection, the count
// Every sum has a fixed shape: no floating-point atomics, no dependence on the launch geometry.
#include "mdvt_internal.h"
#include "mdvt_adapter_resize.h"
#include "mdvt_depth_code.h"
#include "mdvt_pairwise.h"

namespace mdvt {
namespace {

using depth_code::store_plane;
using depth_code::tap;
using pairwise::kChunk;

// ---- mdvt_model_frames ---------------------------------------------------------------------------------------------------------

template <bool AS_FLOAT>
__global__ void __launch_bounds__(256) k_model_frames(ModelFramesArgs a)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= a.groups) return;
    const uint32_t row = t / a.gw, g = t - row * a.gw;
    const int x0 = (int)(4u * g);
    const int nv = a.rs.out_w - x0 < 4 ? a.rs.out_w - x0 : 4;
    const size_t f = (size_t)a.frame0 + blockIdx.y;
    const uint8_t* src = a.src + f * a.src_stride;
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
    uint8_t* out = a.dst + f * a.dst_stride + (size_t)row * a.dst_pitch + (size_t)x0 * (AS_FLOAT ? 4u : 1u);
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

template <bool RESIZE>
__global__ void __launch_bounds__(256) k_depth_prompt(DepthPromptArgs a)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= a.groups) return;
    const uint32_t row = t / a.gw, g = t - row * a.gw;
    const int x0 = (int)(4u * g);
    const int nv = a.out_w - x0 < 4 ? a.out_w - x0 : 4;
    const size_t f = (size_t)a.frame0 + blockIdx.y;
    const uint8_t* src = a.src + f * a.src_stride;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    if (!RESIZE) {
        const uint8_t* r = src + (size_t)row * a.src_pitch;
        if (a.src_vec && nv == 4) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(r + (size_t)x0 * 3u);
            uint32_t px[4];
            unpack4(q[0], q[1], q[2], px);
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = decode_px(px[k], a.bgr, a.mult);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nv) d[k] = decode_px(load_px_bytes(r, x0 + k), a.bgr, a.mult);
        }
    } else {
        int y0, y1;
        float b0, b1;
        tap((int)row, a.ratio_y, a.in_h, y0, y1, b0, b1);
        const uint8_t* r0 = src + (size_t)y0 * a.src_pitch;
        const uint8_t* r1 = src + (size_t)y1 * a.src_pitch;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < nv) {
                int s0, s1;
                float a0, a1;
                tap(x0 + k, a.ratio_x, a.in_w, s0, s1, a0, a1);
                const float h0 = decode_px(load_px_bytes(r0, s0), a.bgr, a.mult) * a0 + decode_px(load_px_bytes(r0, s1), a.bgr, a.mult) * a1;
                const float h1 = decode_px(load_px_bytes(r1, s0), a.bgr, a.mult) * a0 + decode_px(load_px_bytes(r1, s1), a.bgr, a.mult) * a1;
                d[k] = h0 * b0 + h1 * b1;
            }
        }
    }
    store_plane(reinterpret_cast<float*>(a.dst + f * a.dst_stride + (size_t)row * a.dst_pitch) + x0, d, nv, a.dst_vec != 0);
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
    const int lane = (int)threadIdx.x;
    const size_t l = blockIdx.x;                                     // the list
    const uint32_t* cnt = a.unit_cnt + l * a.nunits;
    uint32_t* off = a.unit_off + l * a.nunits;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < a.nunits; base += 64u) {
        const uint32_t i = base + (uint32_t)lane;
        const uint32_t v = i < a.nunits ? cnt[i] : 0u;
        uint32_t s = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(s, d);
            if (lane >= d) s += t;
        }
        if (i < a.nunits) off[i] = carry + s - v;
        carry += __shfl(s, 63);
    }
    if (lane == 0) a.totals[l] = carry;
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
    const uint32_t l = blockIdx.x * 64u + threadIdx.x;
    if (l >= 2u * (uint32_t)a.n_frames) return;
    const uint32_t total = a.totals[l];
    const uint32_t nch = (total + (uint32_t)kChunk - 1u) / (uint32_t)kChunk;
    const float* sums = a.sums + (size_t)l * a.nchunks;
    float acc = 0.f;
    for (uint32_t j = 0; j < nch; ++j) acc += sums[j];
    a.focal[l] = total ? acc / (float)total : 0.0f;                  // unik3d_video.py:98-99
    if (a.counts) a.counts[l] = total;
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
    hipLaunchKernelGGL(k_focal_mean, dim3((lists + 63u) / 64u), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdvt
