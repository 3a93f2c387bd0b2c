// mdvt_metric_align.hip -- relative inverse depth to metric depth codes (mdvt_scale_shift_fit, mdvt_metric_depth_codes;
// include/mdvt_metric_align.h): the reference's compute_scale_and_shift_full (vmc:17-41), its per-pixel inverse (vmc:136-142,
// dcv:236-243) and save_depth_video's resize and 16-bit code (dfh:5-11, 48-61, 153), bit for bit.
//
// The unit is compiled with -ffp-contract=off, -fhip-fp32-correctly-rounded-divide-sqrt and without fast-math (Makefile): every
// `*`, `+` and `/` below is one IEEE operation, rounded before the next.
//
// The fit.  Five float32 sums over the n = n_frames * H * W values of the concatenated planes, each in NumPy's order
// (mdvt_pairwise.h): with m = float(mask byte) or 1, p the prediction and t the target (or 1 / target),
//     (m p) p,   m p,   m,   (m p) t,   m t.
// Logical element e is frame e / (H W), row (e % (H W)) / W, column e % W of a pitched plane, so a chunk or a leaf may start in the
// middle of a row and end in the next frame.
//   k_fit_chunks  one workgroup of four waves per chunk of 8192 elements.  A full chunk is staged in LDS in two halves of 32 leaves
//                 (16-byte loads of four elements where the plane's layout allows, element by element otherwise; 8 dwords of padding
//                 per leaf, so that the 32 lanes of a read -- 4 leaves x 8 accumulators -- hit 32 banks).  Thread 8 l + k keeps
//                 accumulator k of leaf l for all five sums: 16 elements in order; butterfly steps 1, 2, 4 join a leaf as
//                 ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), steps 8, 16, 32 the wave's 8 leaves, thread 0 the four waves and the two halves:
//                 the balanced tree (IEEE add is commutative: both sides of a step hold the same bits).  The tail chunk is walked in
//                 the general shape straight from global memory, all five sums in one pass, eight threads per leaf.
//   k_fit_total   one workgroup of five waves, a wave per sum: the set's chunk sums added in order onto the running totals; after the
//                 last set det, scale and shift.
//
// The codes.  k_metric_codes: a thread per four output pixels of a row, in the frame, gather and tail of mdvt_depth_code.h (quad_of,
// quad_values, codes_out), which mdvt_depth_sink.hip uses too; this unit's own is reconstruct, the function of a source value.  Same
// size: reconstruct, clip, code.  Resized: each output pixel reconstructs its up to four source values (they come from L1/L2: a 2 x
// upscale reads every source value four times, but the kernel's traffic to memory stays the algorithmic 4 B per source and 3 B per
// output pixel), filters horizontally then vertically, clips and codes.  Four codes are 12 bytes: three dword stores where the
// image's address, pitch and stride are multiples of 4.
#include "mdvt_internal.h"
#include "mdvt_pairwise.h"
#include "mdvt_depth_code.h"

namespace mdvt {
namespace {

using pairwise::kChunk;
using pairwise::kLeaf;
using depth_code::clip_np;
using depth_code::Quad;
using depth_code::quad_of;
using depth_code::quad_values;
using depth_code::codes_out;

constexpr int kFitThreads = 256;
constexpr int kTotalThreads = 5 * 64;              // k_fit_total: a wave per sum
constexpr int kHalf = kChunk / 2;                 // elements staged at once: 32 leaves, one accumulator per thread
constexpr int kLeafStride = kLeaf + 8;            // dwords per staged leaf
constexpr int kStaged = (kHalf / kLeaf) * kLeafStride;

struct Elem { float p, t, m; };

// the address of logical element e of a plane of `size`-byte values
__device__ __forceinline__ const uint8_t* elem_at(const FitPlane& pl, uint32_t e, uint32_t size)
{
    uint32_t f = 0, row = 0, col = e;
    if (pl.W != pl.n) {                           // (a plane without padding is one long row: no division)
        f = e / pl.HW;
        const uint32_t r = e - f * pl.HW;
        row = r / pl.W;
        col = r - row * pl.W;
    }
    return pl.p + (size_t)f * pl.stride + (size_t)row * pl.pitch + (size_t)col * size;
}

__device__ __forceinline__ Elem load_elem(const FitArgs& a, uint32_t e)
{
    Elem v;
    v.p = *reinterpret_cast<const float*>(elem_at(a.pred, e, 4u));
    v.t = *reinterpret_cast<const float*>(elem_at(a.target, e, 4u));
    if (a.target_is_depth) v.t = 1.0f / v.t;
    v.m = a.mask.p ? (float)*elem_at(a.mask, e, 1u) : 1.0f;
    return v;
}

// sum `which` of the five: the value element e contributes
__device__ __forceinline__ float fit_value(const Elem& v, int which)
{
    const float mp = v.m * v.p;
    switch (which) {
    case 0: return mp * v.p;
    case 1: return mp;
    case 2: return v.m;
    case 3: return mp * v.t;
    default: return v.m * v.t;
    }
}

// four values e .. e + 3 of a float plane (e a multiple of 4, all four inside the plane)
__device__ __forceinline__ float4 load_f4(const FitPlane& pl, uint32_t e)
{
    if (pl.vec) return *reinterpret_cast<const float4*>(elem_at(pl, e, 4u));
    float4 o;
    o.x = *reinterpret_cast<const float*>(elem_at(pl, e, 4u));
    o.y = *reinterpret_cast<const float*>(elem_at(pl, e + 1u, 4u));
    o.z = *reinterpret_cast<const float*>(elem_at(pl, e + 2u, 4u));
    o.w = *reinterpret_cast<const float*>(elem_at(pl, e + 3u, 4u));
    return o;
}

__device__ __forceinline__ uint32_t load_b4(const FitPlane& pl, uint32_t e)
{
    if (pl.vec) return *reinterpret_cast<const uint32_t*>(elem_at(pl, e, 1u));
    return (uint32_t)*elem_at(pl, e, 1u) | ((uint32_t)*elem_at(pl, e + 1u, 1u) << 8) | ((uint32_t)*elem_at(pl, e + 2u, 1u) << 16) |
           ((uint32_t)*elem_at(pl, e + 3u, 1u) << 24);
}

__device__ __forceinline__ int staged_at(int i) { return (i >> 7) * kLeafStride + (i & (kLeaf - 1)); }

__global__ void __launch_bounds__(kFitThreads) k_fit_chunks(FitArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_p[kStaged];
    __shared__ __attribute__((aligned(16))) float s_t[kStaged];
    __shared__ __attribute__((aligned(16))) uint8_t s_m[kStaged];
    __shared__ pairwise::Shape s_shape;
    __shared__ float s_wave[4][5], s_half[5];
    // a short chunk stages nothing: its leaf sums and join stacks, per sum, take the staging arrays' place
    static_assert(5 * kLeaf <= kStaged && 5 * 16 <= kStaged, "the short chunk's arrays fit the staging arrays");
    float (*s_leaf)[kLeaf] = reinterpret_cast<float (*)[kLeaf]>(s_p);
    float (*s_val)[16] = reinterpret_cast<float (*)[16]>(s_t);
    uint8_t (*s_depth)[16] = reinterpret_cast<uint8_t (*)[16]>(s_m);
    const int tid = (int)threadIdx.x;
    const uint32_t c = a.chunk0 + blockIdx.x;
    const uint32_t first = c * (uint32_t)kChunk;                 // < n < 2^31
    const int n = (int)(a.n - first < (uint32_t)kChunk ? a.n - first : (uint32_t)kChunk);
    float* out = a.sums + blockIdx.x;                            // sum w of this chunk: out[w * sums_stride]
    const bool masked = a.mask.p != nullptr;

    if (n < kChunk) {
        // the general shape (mdvt_pairwise.h), all five sums in one pass over the elements: thread 8 l + k keeps accumulator k of leaf l
        // (a leaf of fewer than 8 values -- a chunk of fewer than 8 -- is summed in order by its first thread), butterfly steps 1, 2, 4
        // join the leaf, its first thread adds the last n % 8 values in order; then a thread per sum joins the leaves
        if (tid == 0) pairwise::shape_list(s_shape, n);
        __syncthreads();
        const int k = tid & 7;
        for (int l = tid >> 3; l < s_shape.leaves; l += kFitThreads / 8) {
            const uint32_t at = first + s_shape.leaf_at[l];
            const int m = s_shape.leaf_n[l], m8 = m - m % 8;
            float r[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            if (m8) {
                {
                    const Elem v = load_elem(a, at + (uint32_t)k);
#pragma unroll
                    for (int w = 0; w < 5; ++w) r[w] = fit_value(v, w);
                }
#pragma unroll 4
                for (int i = 8; i < m8; i += 8) {
                    const Elem v = load_elem(a, at + (uint32_t)(i + k));
#pragma unroll
                    for (int w = 0; w < 5; ++w) r[w] += fit_value(v, w);
                }
#pragma unroll
                for (int w = 0; w < 5; ++w) {
#pragma unroll
                    for (int x = 1; x < 8; x <<= 1) r[w] += __shfl_xor(r[w], x);
                }
            }
            if (k == 0) {
                for (int i = m8; i < m; ++i) {
                    const Elem v = load_elem(a, at + (uint32_t)i);
#pragma unroll
                    for (int w = 0; w < 5; ++w) r[w] += fit_value(v, w);
                }
#pragma unroll
                for (int w = 0; w < 5; ++w) s_leaf[w][l] = r[w];
            }
        }
        __syncthreads();
        if (tid < 5) out[(size_t)tid * a.sums_stride] = pairwise::shape_join(s_shape, s_leaf[tid], s_val[tid], s_depth[tid]);
        return;
    }

    for (int h = 0; h < 2; ++h) {
        if (h) __syncthreads();                                  // (the first half has been read)
#pragma unroll
        for (int g = 0; g < kHalf / (4 * kFitThreads); ++g) {
            const int i = 4 * (g * kFitThreads + tid);
            const uint32_t e = first + (uint32_t)(h * kHalf + i);
            const float4 p = load_f4(a.pred, e);
            float4 t = load_f4(a.target, e);
            if (a.target_is_depth) { t.x = 1.0f / t.x; t.y = 1.0f / t.y; t.z = 1.0f / t.z; t.w = 1.0f / t.w; }
            *reinterpret_cast<float4*>(s_p + staged_at(i)) = p;
            *reinterpret_cast<float4*>(s_t + staged_at(i)) = t;
            if (masked) *reinterpret_cast<uint32_t*>(s_m + staged_at(i)) = load_b4(a.mask, e);
        }
        __syncthreads();
        // thread 8 l + k: accumulator k of leaf l
        const int at = (tid >> 3) * kLeafStride + (tid & 7);
        float r[5];
        {
            const Elem v{s_p[at], s_t[at], masked ? (float)s_m[at] : 1.0f};
#pragma unroll
            for (int w = 0; w < 5; ++w) r[w] = fit_value(v, w);
        }
#pragma unroll
        for (int i = 1; i < kLeaf / 8; ++i) {
            const int j = at + 8 * i;
            const Elem v{s_p[j], s_t[j], masked ? (float)s_m[j] : 1.0f};
#pragma unroll
            for (int w = 0; w < 5; ++w) r[w] += fit_value(v, w);
        }
#pragma unroll
        for (int w = 0; w < 5; ++w) {
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) r[w] += __shfl_xor(r[w], m);
        }
        if ((tid & 63) == 0) {
#pragma unroll
            for (int w = 0; w < 5; ++w) s_wave[tid >> 6][w] = r[w];
        }
        __syncthreads();
        if (tid < 5) {
            const float v = (s_wave[0][tid] + s_wave[1][tid]) + (s_wave[2][tid] + s_wave[3][tid]);
            if (h == 0) s_half[tid] = v;
            else out[(size_t)tid * a.sums_stride] = s_half[tid] + v;
        }
    }
}

// One wave per sum (wave w adds sum w), so the five chains run side by side.  The wave first brings its sum's values of the set into
// LDS, all loads in flight at once (a lane past the end reads value 0 again: no branch), then walks them 64 at a time: a chain's step
// is a lane read with a constant lane number (the value comes through a scalar register) and the add that depends on it.  Every
// lane of a wave carries the same running total.
__global__ void __launch_bounds__(kTotalThreads) k_fit_total(FitArgs a)
{
    __shared__ float s_sums[5][kFitSetChunks];
    __shared__ float s_acc[5];
    const uint32_t lane = threadIdx.x & 63u;
    const int w = (int)(threadIdx.x >> 6);
    const uint32_t n = a.nchunks_set;                            // 1 .. kFitSetChunks
    const float* sums = a.sums + (size_t)w * a.sums_stride;
    float v[kFitSetChunks / 64];
#pragma unroll
    for (uint32_t k = 0; k < kFitSetChunks / 64u; ++k) {
        const uint32_t i = 64u * k + lane;
        v[k] = sums[i < n ? i : 0u];
    }
#pragma unroll
    for (uint32_t k = 0; k < kFitSetChunks / 64u; ++k) s_sums[w][64u * k + lane] = v[k];
    __syncthreads();
    float r = a.first_set ? 0.f : a.state[w];
    for (uint32_t base = 0; base < n; base += 64u) {
        const float s = s_sums[w][base + lane];
        if (n - base >= 64u) {
            const int bits = __float_as_int(s);
#pragma unroll
            for (int j = 0; j < 64; ++j) r += __int_as_float(__builtin_amdgcn_readlane(bits, j));
        } else {
            const int m = (int)(n - base);
            for (int j = 0; j < m; ++j) r += __shfl(s, j);
        }
    }
    if (lane == 0) s_acc[w] = r;
    __syncthreads();
    if (threadIdx.x != 0) return;
    float acc[5];
    for (int k = 0; k < 5; ++k) acc[k] = s_acc[k];
    if (!a.last_set) {
        for (int w = 0; w < 5; ++w) a.state[w] = acc[w];
        return;
    }
    const float a00 = acc[0], a01 = acc[1], a11 = acc[2], b0 = acc[3], b1 = acc[4];
    const float det = a00 * a11 - a01 * a01;
    float scale = 1.0f, shift = 0.0f;
    if (det != 0.0f) {                                           // (a NaN is)
        scale = (a11 * b0 - a01 * b1) / det;
        shift = (-a01 * b0 + a00 * b1) / det;
    }
    a.out[0] = a00; a.out[1] = a01; a.out[2] = a11; a.out[3] = b0; a.out[4] = b1;
    a.out[5] = scale; a.out[6] = shift; a.out[7] = det;
}

// ---- the codes ----------------------------------------------------------------------------------------------------------------

template <int STYLE>
__device__ __forceinline__ float reconstruct(float x, float scale, float shift, float fmax)
{
    float inv = x * scale + shift;                               // (two roundings: the unit is compiled without contraction)
    if (STYLE == 0) {
        const float d = 1.0f / inv;
        return d < 0.0f ? fmax : d;
    }
    if (inv == 0.0f) inv = 1e-4f;
    const float d = clip_np(1.0f / inv, fmax);
    return d != d ? fmax : d;
}

template <int STYLE>
__global__ void __launch_bounds__(256) k_metric_codes(DepthCodesArgs a)
{
    Quad q;
    if (!quad_of(a.groups, a.gw, a.out_w, a.frame0, q)) return;
    const float scale = a.scale_shift[0], shift = a.scale_shift[1], fmax = a.fmax;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    quad_values(d, a.src + q.f * a.src_stride, a.src_pitch, a.src_vec != 0, q, a.resize != 0, a.ratio_x, a.ratio_y, a.in_w, a.in_h,
                [=](float x) { return reconstruct<STYLE>(x, scale, shift, fmax); });
    if (STYLE == 1 && a.resize) {                                // (style 1 clips the filtered value too)
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = clip_np(d[k], fmax);
    }
    codes_out(d, q, a);
}

}  // namespace

hipError_t launch_scale_shift_fit(const FitArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_fit_chunks, dim3(a.nchunks_set), dim3(kFitThreads), 0, s, a);
    hipLaunchKernelGGL(k_fit_total, dim3(1), dim3(kTotalThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_metric_codes(const DepthCodesArgs& a, int n_frames, hipStream_t s)
{
    const dim3 grid((a.groups + 255u) / 256u, (unsigned)n_frames);
    if (a.style == 0) hipLaunchKernelGGL(k_metric_codes<0>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_metric_codes<1>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdvt
