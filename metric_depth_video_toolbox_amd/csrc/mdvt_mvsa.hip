// mdvt_mvsa.hip -- the non-model work of the reference's MVSAnywhere step (include/mdvt_mvsa.h): packed video frames to the model's
// planar float32 input through torch's bilinear resize (mdvt_bilinear_model_frames), the refined depth through two nearest-neighbour
// resizes to a depth video's codes (mdvt_nearest_depth_codes) and the masked median ratio between the cost volume's depth and the
// refined depth (mdvt_ratio_median).
//
// The unit is compiled with -ffp-contract=off, IEEE division and without fast-math (Makefile): every `*`, `+`, `-` and `/` below is
// one IEEE operation, rounded before the next.  Shared with other units through mdvt_depth_code.h: the four-pixel frame (quad_of), the
// plane stores (store_plane) and the tail of the code kernels (codes_out: NumPy's clip, the 16-bit code, the packed stores).
//
// k_bilinear_frames, k_nearest_codes: a thread per four output pixels of a row, a frame per blockIdx.y.  The bilinear taps are gathered
// byte by byte: the taps of neighbouring pixels are neighbours or the same, and the caches serve them.  The 256 values v / 255 are
// divided once per workgroup, one per thread, into LDS: a tap is a table look-up, the same bits as its own division.  The planar
// stores are 16 bytes per lane where the layout allows, neighbouring lanes neighbouring addresses.  A value's arithmetic does not
// depend on which stores it takes.
//
// The median per launch set, after the set's scratch has been zeroed: four times
//   k_median_hist  workgroups stride over a frame's pixels: validity and ratio of each, the ratios that share the digits chosen so far
//                  counted by their next 8 bits in an LDS histogram, the histogram merged into the frame's with integer atomics
//   k_median_pick  one workgroup per frame: the inclusive scan of the 256 counts, the digit whose span holds the sought index, the
//                  histogram zeroed for the next pass; the last pass writes the median and the count
// Counts are integers and the walk is over digits: no sort, no floating-point atomic, no dependence on the launch geometry.
#include "mdvt_internal.h"
#include "mdvt_device.h"
#include "mdvt_depth_code.h"
#include "mdvt_torch_resize.h"

namespace mdvt {
namespace {

using depth_code::store_plane;
using depth_code::Quad;
using depth_code::quad_of;
using depth_code::codes_out;
using torch_resize::lin_tap;                                        // the bilinear taps and the two forms of their sum: mdvt_torch_resize.h
using torch_resize::lin_mix;

// torch's CPU nearest map (include/mdvt_mvsa.h): index x of n_out values -> its source among n_in, scale = fl(float(n_in) / float(n_out))
__device__ __forceinline__ int near_idx(uint32_t x, float scale, int n_in)
{
    const float f = floorf((float)x * scale);
    return f >= (float)(n_in - 1) ? n_in - 1 : (int)f;              // (x and scale are >= 0: so is f)
}

__device__ __forceinline__ int near_twice(uint32_t x, const NearAxis& ax)
{
    return near_idx((uint32_t)near_idx(x, ax.to_mid, ax.mid), ax.to_src, ax.src);
}

// ---- mdvt_bilinear_model_frames ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_bilinear_frames(BilinearFramesArgs a)
{
    __shared__ float s_unit[256];                                   // fl(float(v) / 255.0f) of every byte v: one division each
    s_unit[threadIdx.x] = (float)threadIdx.x / 255.0f;
    __syncthreads();
    Quad q;
    if (!quad_of(a.groups, a.gw, a.out_w, a.frame0, q)) return;
    int y0, y1;
    float wy0, wy1;
    lin_tap((int)q.row, a.scale_y, a.in_h, y0, y1, wy0, wy1);
    const uint8_t* frame = a.src + q.f * a.src_stride;
    const uint8_t* r0 = frame + (size_t)y0 * a.src_pitch;
    const uint8_t* r1 = frame + (size_t)y1 * a.src_pitch;
    float v[3][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < q.nv) {
            int x0, x1;
            float wx0, wx1;
            lin_tap(q.x0 + k, a.scale_x, a.in_w, x0, x1, wx0, wx1);
            const uint32_t p00 = load_px_bytes(r0, x0), p01 = load_px_bytes(r0, x1);
            const uint32_t p10 = load_px_bytes(r1, x0), p11 = load_px_bytes(r1, x1);
#pragma unroll
            for (int c = 0; c < 3; ++c) {                           // planes R, G, B
                const int shift = 8 * (a.bgr ? 2 - c : c);
                const float v00 = s_unit[(p00 >> shift) & 0xFFu], v01 = s_unit[(p01 >> shift) & 0xFFu];
                const float v10 = s_unit[(p10 >> shift) & 0xFFu], v11 = s_unit[(p11 >> shift) & 0xFFu];
                v[c][k] = lin_mix(a.small != 0, wy0, wy1, wx0, wx1, v00, v01, v10, v11);
            }
        }
    }
    uint8_t* out = a.dst + q.f * a.dst_stride + (size_t)q.row * a.dst_pitch + (size_t)q.x0 * 4u;
#pragma unroll
    for (int c = 0; c < 3; ++c) store_plane(reinterpret_cast<float*>(out + (size_t)c * a.dst_plane), v[c], q.nv, a.dst_vec != 0);
}

// ---- mdvt_nearest_depth_codes --------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_nearest_codes(NearestCodesArgs a)
{
    Quad q;
    if (!quad_of(a.c.groups, a.c.gw, a.c.out_w, a.c.frame0, q)) return;
    const int sy = near_twice(q.row, a.y);
    const float* row = reinterpret_cast<const float*>(a.c.src + q.f * a.c.src_stride + (size_t)sy * a.c.src_pitch);
    const bool scaled = a.scales != nullptr;
    const float s = scaled ? *reinterpret_cast<const float*>(a.scales + q.f * a.scales_stride) : 1.0f;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < q.nv) {
            const float x = row[near_twice((uint32_t)(q.x0 + k), a.x)];
            d[k] = scaled ? x * s : x;
        }
    }
    codes_out(d, q, a.c);
}

// ---- mdvt_ratio_median ---------------------------------------------------------------------------------------------------------

constexpr float kRatioEps = 1e-6f;                                  // float32(1e-6) (video_mvsa.py:286: a float32 tensor plus a Python float)
constexpr unsigned kMedianBlocks = 64;                              // workgroups per frame of a histogram pass, at the most

// pixel p < npx of frame f of the set, in row-major order: is it valid, and the bits of its ratio (video_mvsa.py:283-290)
__device__ __forceinline__ bool ratio_bits(const RatioMedianArgs& a, size_t f, uint32_t p, uint32_t& bits)
{
    const uint32_t y = p / a.cv_w, x = p - y * a.cv_w;
    if (a.mask) {
        const uint8_t* m = a.mask + f * a.mask_stride + (size_t)near_idx(y, a.mask_sy, a.mask_h) * a.mask_pitch;
        if (m[near_idx(x, a.mask_sx, a.mask_w)] == 0) return false;
    }
    const float cv = reinterpret_cast<const float*>(a.cv + f * a.cv_stride + (size_t)y * a.cv_pitch)[x];
    const float ref = reinterpret_cast<const float*>(a.ref + f * a.ref_stride + (size_t)near_idx(y, a.ref_sy, a.ref_h) * a.ref_pitch)[near_idx(x, a.ref_sx, a.ref_w)];
    const bool fin = fabsf(cv) < INFINITY && fabsf(ref) < INFINITY;     // (a NaN compares false)
    if (!(fin && cv > 0.0f && ref > 0.0f)) return false;
    float r = cv / (ref + kRatioEps);
    r = r < 0.0f ? 0.0f : r;                                        // clamp_min(0): r is >= 0 already, +0 or +inf included
    bits = __float_as_uint(r);
    return true;
}

__global__ void __launch_bounds__(256) k_median_hist(RatioMedianArgs a, int pass)
{
    __shared__ uint32_t s_hist[256];
    const size_t f = blockIdx.y;
    uint32_t* w = a.work + f * kMedianFrameWords;
    const uint32_t prefix = w[256], count = w[258];
    if (pass > 0 && count == 0) return;                             // (uniform: the whole workgroup leaves)
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < a.npx; p += gridDim.x * 256u) {
        uint32_t bits;
        if (!ratio_bits(a, f, p, bits)) continue;
        if (pass == 0 || (bits >> (shift + 8)) == prefix) atomicAdd(&s_hist[(bits >> shift) & 0xFFu], 1u);
    }
    __syncthreads();
    const uint32_t n = s_hist[threadIdx.x];
    if (n) atomicAdd(&w[threadIdx.x], n);
}

__global__ void __launch_bounds__(256) k_median_pick(RatioMedianArgs a, int pass)
{
    __shared__ uint32_t s_scan[256];
    const uint32_t t = threadIdx.x;
    const size_t f = blockIdx.x;
    uint32_t* w = a.work + f * kMedianFrameWords;
    const uint32_t h = w[t];
    const uint32_t prefix = w[256];
    uint32_t k = w[257], count = w[258];
    uint32_t incl = h;
    s_scan[t] = incl;
    __syncthreads();
    for (uint32_t d = 1; d < 256u; d <<= 1) {                       // the inclusive scan of the 256 counts
        const uint32_t add = t >= d ? s_scan[t - d] : 0u;
        __syncthreads();
        incl += add;
        s_scan[t] = incl;
        __syncthreads();
    }
    if (pass == 0) {
        count = s_scan[255];
        k = count ? (count - 1u) / 2u : 0u;                         // the lower median's place in the sorted sequence
    }
    w[t] = 0;                                                       // (h is in a register: the next pass counts from zero)
    const uint32_t excl = incl - h;
    if (count != 0 && h != 0 && excl <= k && k < incl) {            // exactly one digit's span holds k
        const uint32_t chosen = (prefix << 8) | t;
        w[256] = chosen;
        w[257] = k - excl;
        if (pass == 3) a.median[f] = __uint_as_float(chosen);
    }
    if (t == 0) {
        if (pass == 0) w[258] = count;
        if (pass == 3) {
            if (count == 0) a.median[f] = 1.0f;                     // video_mvsa.py:292-293
            if (a.counts) a.counts[f] = count;
        }
    }
}

}  // namespace

hipError_t launch_bilinear_frames(const BilinearFramesArgs& a, int n_frames, hipStream_t s)
{
    const dim3 grid((a.groups + 255u) / 256u, (unsigned)n_frames);
    hipLaunchKernelGGL(k_bilinear_frames, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_nearest_codes(const NearestCodesArgs& a, int n_frames, hipStream_t s)
{
    const dim3 grid((a.c.groups + 255u) / 256u, (unsigned)n_frames);
    hipLaunchKernelGGL(k_nearest_codes, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ratio_median(const RatioMedianArgs& a, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(a.work, 0, (size_t)a.n_frames * kMedianFrameWords * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const unsigned need = (a.npx + 255u) / 256u;
    const dim3 hist(need < kMedianBlocks ? need : kMedianBlocks, (unsigned)a.n_frames);
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(k_median_hist, hist, dim3(256), 0, s, a, pass);
        hipLaunchKernelGGL(k_median_pick, dim3((unsigned)a.n_frames), dim3(256), 0, s, a, pass);
    }
    return hipGetLastError();
}

}  // namespace mdvt
