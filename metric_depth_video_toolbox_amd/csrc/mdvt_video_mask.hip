// mdvt_video_mask.hip -- the device work of the mask-video step around its model (include/mdvt_video_mask.h): Pillow's
// Image.resize(LANCZOS) on 8-bit pixels, rembg's normalize in front of the network and its predict's tail behind it.
//
// The resampler.  The coefficient and bounds tables of both axes come from the host (mdvt_lanczos_table.h: double arithmetic, the C
// library's sin); what runs here is integer: out = clamp(((1 << 21) + sum in[first + x] * k[x]) >> 22, 0, 255) in int32, the
// horizontal pass first, into a uint8 image, then the vertical pass on that image.  A table is stored tap-major (k[x][out]), so the
// lanes of a wave, which take neighbouring outputs, read neighbouring words.  No sum's order is free (integer), nothing is
// accumulated across threads: the result cannot depend on the launch geometry.
//
//   k_lz_rows   the horizontal pass: a thread per (row, output column), its 1 or 3 channels; 64 columns x 4 rows per workgroup.  The
//               source windows of neighbouring columns overlap or adjoin: a wave's byte loads fall into one run of a row.
//   k_lz_cols   the vertical pass: a thread per (output row, byte of that row); the 64 lanes of a wave read 64 neighbouring bytes
//               of every source row and share the tap, whose word is one broadcast load.
//   k_lz_fused  both passes in one workgroup per (frame, strip of kLzStrip output columns): the horizontal pass of the whole strip
//               goes into LDS as uint8 [in_h][kLzStrip * C] (a 1080-row RGB frame: 26 KB; at most kLzFusedLds), the vertical pass
//               reads it from there: the intermediate image never exists in global memory.  A row of the strip is 8 or 24 bytes, so
//               the lanes of a wave read 64 neighbouring bytes of LDS (16 banks, four lanes to a dword: a broadcast, no conflict).
//   k_lz_copy   both passes skipped (equal sizes).
// With rep = 3 (C = 1) the pass that writes the result writes every value as three equal bytes: the grey frame of a mask video.
//
// rembg's normalize: k_u8_max takes the frame's maximum byte (an integer atomicMax per workgroup), k_mask_lut makes the frame's
// 3 x 256 values float32((double(v) / m - mean[c]) / std[c]) -- two IEEE double divisions, one rounding --, k_mask_planar looks every
// byte up, four pixels of a row per thread, 16-byte stores where the planes are aligned.  predict's tail: k_pred_minmax takes the
// plane's float32 minimum and maximum through order-preserving integer keys (exact, order-free) and flags a NaN or an infinity,
// k_pred_bytes writes trunc(fl(fl(fl(x - mi) / fl(ma - mi)) * 255.0f)).  The unit is compiled with -ffp-contract=off and IEEE division.
#include "mdvt_internal.h"
#include "mdvt_depth_code.h"

namespace mdvt {
namespace {

using depth_code::store_plane;

constexpr int kLzRound = 1 << 21;

__device__ __forceinline__ uint8_t lz_clip8(int v)
{
    v >>= 22;                                                        // arithmetic
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

__device__ __forceinline__ void lz_store(uint8_t* o, uint8_t v, int rep)
{
    o[0] = v;
    if (rep == 3) { o[1] = v; o[2] = v; }
}

// ---- the two-launch form ---------------------------------------------------------------------------------------------------------

template <int C>
__global__ void __launch_bounds__(256) k_lz_rows(LzArgs a)
{
    const int xx = (int)(blockIdx.x * 64u + (threadIdx.x & 63u));
    const int row = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (xx >= a.out_w || row >= a.in_h) return;
    const size_t f = blockIdx.z;
    const int first = a.h.bounds[2 * xx], taps = a.h.bounds[2 * xx + 1];
    const uint8_t* r = a.src + f * a.src_stride + (size_t)row * a.src_pitch + (size_t)first * C;
    const int32_t* k = a.h.coef + xx;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = kLzRound;
    for (int x = 0; x < taps; ++x) {
        const int kx = k[(size_t)x * (size_t)a.out_w];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += (int)r[x * C + c] * kx;
    }
    uint8_t* o = a.dst + f * a.dst_stride + (size_t)row * a.dst_pitch + (size_t)xx * C * a.rep;
#pragma unroll
    for (int c = 0; c < C; ++c) lz_store(o + c * a.rep, lz_clip8(acc[c]), a.rep);
}

__global__ void __launch_bounds__(256) k_lz_cols(LzArgs a)
{
    const int wb = a.out_w * a.C;                                    // bytes of a row
    const int j = (int)(blockIdx.x * 64u + (threadIdx.x & 63u));
    const int yy = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (j >= wb || yy >= a.out_h) return;
    const size_t f = blockIdx.z;
    const int first = a.v.bounds[2 * yy], taps = a.v.bounds[2 * yy + 1];
    const uint8_t* p = a.src + f * a.src_stride + (size_t)first * a.src_pitch + j;
    const int32_t* k = a.v.coef + yy;
    int acc = kLzRound;
    for (int y = 0; y < taps; ++y) acc += (int)p[(size_t)y * a.src_pitch] * k[(size_t)y * (size_t)a.out_h];
    lz_store(a.dst + f * a.dst_stride + (size_t)yy * a.dst_pitch + (size_t)j * a.rep, lz_clip8(acc), a.rep);
}

__global__ void __launch_bounds__(256) k_lz_copy(LzArgs a)
{
    const int wb = a.out_w * a.C;
    const int j = (int)(blockIdx.x * 64u + (threadIdx.x & 63u));
    const int yy = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (j >= wb || yy >= a.out_h) return;
    const size_t f = blockIdx.z;
    lz_store(a.dst + f * a.dst_stride + (size_t)yy * a.dst_pitch + (size_t)j * a.rep,
             a.src[f * a.src_stride + (size_t)yy * a.src_pitch + j], a.rep);
}

// ---- the fused form --------------------------------------------------------------------------------------------------------------

template <int C>
__global__ void __launch_bounds__(256) k_lz_fused(LzArgs a)
{
    extern __shared__ __align__(16) uint8_t s_img[];                 // [in_h][kLzStrip * C]
    constexpr int RB = kLzStrip * C;
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * kLzStrip;
    const int sw = a.out_w - x0 < kLzStrip ? a.out_w - x0 : kLzStrip;          // >= 1: the grid has ceil(out_w / kLzStrip) strips
    const size_t f = blockIdx.y;
    const uint8_t* src = a.src + f * a.src_stride;
    for (int i = tid; i < a.in_h * sw; i += 256) {
        const int row = i / sw, col = i - row * sw, xx = x0 + col;
        const int first = a.h.bounds[2 * xx], taps = a.h.bounds[2 * xx + 1];
        const uint8_t* r = src + (size_t)row * a.src_pitch + (size_t)first * C;
        const int32_t* k = a.h.coef + xx;
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = kLzRound;
        for (int x = 0; x < taps; ++x) {
            const int kx = k[(size_t)x * (size_t)a.out_w];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += (int)r[x * C + c] * kx;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) s_img[row * RB + col * C + c] = lz_clip8(acc[c]);
    }
    __syncthreads();
    const int wb = sw * C;
    uint8_t* dst = a.dst + f * a.dst_stride + (size_t)x0 * C * a.rep;
    for (int i = tid; i < a.out_h * wb; i += 256) {
        const int yy = i / wb, j = i - yy * wb;
        const int first = a.v.bounds[2 * yy], taps = a.v.bounds[2 * yy + 1];
        const uint8_t* p = s_img + first * RB + j;                   // first + taps <= in_h (the table's bounds)
        const int32_t* k = a.v.coef + yy;
        int acc = kLzRound;
        for (int y = 0; y < taps; ++y) acc += (int)p[y * RB] * k[(size_t)y * (size_t)a.out_h];
        lz_store(dst + (size_t)yy * a.dst_pitch + (size_t)j * a.rep, lz_clip8(acc), a.rep);
    }
}

// ---- rembg's normalize -------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_u8_max(MaskInputArgs a)
{
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    const size_t f = blockIdx.y;
    const int wb = a.w * 3;
    uint32_t m = 0u;
    for (int row = (int)blockIdx.x; row < a.h; row += (int)gridDim.x) {
        const uint8_t* r = a.img + f * a.img_stride + (size_t)row * a.img_pitch;
        for (int j = (int)threadIdx.x; j < wb; j += 256) m = r[j] > m ? r[j] : m;
    }
    atomicMax(&s_max, m);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(a.max_byte + f, s_max);
}

__global__ void __launch_bounds__(256) k_mask_lut(MaskInputArgs a)
{
    const size_t f = blockIdx.x;
    const uint32_t mb = a.max_byte[f];
    const double m = mb ? (double)mb : 1e-6;                         // max(np.max(im), 1e-6)
    for (int i = (int)threadIdx.x; i < 768; i += 256) {
        const int c = i >> 8, v = i & 255;
        a.lut[f * 768 + i] = (float)(((double)v / m - a.mean[c]) / a.std[c]);
    }
}

__global__ void __launch_bounds__(256) k_mask_planar(MaskInputArgs a)
{
    const uint32_t gw = ((uint32_t)a.w + 3u) / 4u;
    depth_code::Quad q;
    if (!depth_code::quad_of(gw * (uint32_t)a.h, gw, a.w, 0, q)) return;
    const uint32_t row = q.row;
    const int x0 = q.x0, nv = q.nv;
    const size_t f = q.f;
    const uint8_t* r = a.img + f * a.img_stride + (size_t)row * a.img_pitch + (size_t)x0 * 3u;
    uint8_t px[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) px[k] = k < 3 * nv ? r[k] : (uint8_t)0;
    const float* lut = a.lut + f * 768;
    uint8_t* out = a.dst + f * a.dst_stride + (size_t)row * a.dst_pitch + (size_t)x0 * 4u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                                    // planes R, G, B
        const int at = a.bgr ? 2 - c : c;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = lut[c * 256 + px[3 * k + at]];
        store_plane(reinterpret_cast<float*>(out + (size_t)c * a.dst_plane), v, nv, a.dst_vec != 0);
    }
}

// ---- predict's tail ----------------------------------------------------------------------------------------------------------------

// float32 bits <-> a uint32 that orders as the floats do (-0.0 below +0.0: the two give the same bytes further on)
__device__ __forceinline__ uint32_t ordered_key(uint32_t bits) { return bits & 0x80000000u ? ~bits : bits | 0x80000000u; }
__device__ __forceinline__ float key_value(uint32_t key) { return __uint_as_float(key & 0x80000000u ? key & 0x7FFFFFFFu : ~key); }

__global__ void __launch_bounds__(64) k_pred_init(MaskPredArgs a, int n)
{
    const int f = (int)(blockIdx.x * 64u + threadIdx.x);
    if (f >= n) return;
    a.stats[4 * f] = 0xFFFFFFFFu; a.stats[4 * f + 1] = 0u; a.stats[4 * f + 2] = 0u; a.stats[4 * f + 3] = 0u;
}

__global__ void __launch_bounds__(256) k_pred_minmax(MaskPredArgs a)
{
    __shared__ uint32_t s_min, s_max, s_bad;
    if (threadIdx.x == 0) { s_min = 0xFFFFFFFFu; s_max = 0u; s_bad = 0u; }
    __syncthreads();
    const size_t f = blockIdx.y;
    uint32_t lo = 0xFFFFFFFFu, hi = 0u, bad = 0u;
    for (int row = (int)blockIdx.x; row < a.h; row += (int)gridDim.x) {
        const uint32_t* r = reinterpret_cast<const uint32_t*>(a.pred + f * a.pred_stride + (size_t)row * a.pred_pitch);
        for (int x = (int)threadIdx.x; x < a.w; x += 256) {
            const uint32_t bits = r[x], key = ordered_key(bits);
            bad |= (bits & 0x7F800000u) == 0x7F800000u ? 1u : 0u;
            lo = key < lo ? key : lo;
            hi = key > hi ? key : hi;
        }
    }
    atomicMin(&s_min, lo); atomicMax(&s_max, hi); atomicOr(&s_bad, bad);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(a.stats + 4 * f, s_min); atomicMax(a.stats + 4 * f + 1, s_max); atomicOr(a.stats + 4 * f + 2, s_bad);
    }
}

__global__ void __launch_bounds__(256) k_pred_bytes(MaskPredArgs a)
{
    const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u));
    const int row = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (x >= a.w || row >= a.h) return;
    const size_t f = blockIdx.z;
    const float mi = key_value(a.stats[4 * f]), ma = key_value(a.stats[4 * f + 1]);
    const float range = ma - mi;
    uint8_t b = 0;
    if (!a.stats[4 * f + 2] && range > 0.0f && range <= 3.402823466e+38f) {      // the decrees: ma == mi, a NaN, an infinity, an infinite range
        const float v = *reinterpret_cast<const float*>(a.pred + f * a.pred_stride + (size_t)row * a.pred_pitch + (size_t)x * 4u);
        const float p = (v - mi) / range;
        b = (uint8_t)(int)(p * 255.0f);                              // 0 <= p <= 1
    }
    lz_store(a.dst + f * a.dst_stride + (size_t)row * a.dst_pitch + (size_t)x * a.rep, b, a.rep);
}

dim3 tile_grid(int wide, int high, int n_frames) { return dim3(((unsigned)wide + 63u) / 64u, ((unsigned)high + 3u) / 4u, (unsigned)n_frames); }

}  // namespace

hipError_t launch_lz_rows(const LzArgs& a, int n_frames, hipStream_t s)
{
    const dim3 grid = tile_grid(a.out_w, a.in_h, n_frames);
    if (a.C == 3) hipLaunchKernelGGL(k_lz_rows<3>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_lz_rows<1>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_lz_cols(const LzArgs& a, int n_frames, hipStream_t s)
{
    hipLaunchKernelGGL(k_lz_cols, tile_grid(a.out_w * a.C, a.out_h, n_frames), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_lz_copy(const LzArgs& a, int n_frames, hipStream_t s)
{
    hipLaunchKernelGGL(k_lz_copy, tile_grid(a.out_w * a.C, a.out_h, n_frames), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_lz_fused(const LzArgs& a, int n_frames, hipStream_t s)
{
    const size_t lds = (size_t)a.in_h * (size_t)(kLzStrip * a.C);
    if (lds > kLzFusedLds) return hipErrorInvalidValue;              // (the entry points have checked)
    const dim3 grid(((unsigned)a.out_w + (unsigned)kLzStrip - 1u) / (unsigned)kLzStrip, (unsigned)n_frames);
    if (a.C == 3) hipLaunchKernelGGL(k_lz_fused<3>, grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL(k_lz_fused<1>, grid, dim3(256), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_mask_model_input(const MaskInputArgs& a, int n_frames, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(a.max_byte, 0, (size_t)n_frames * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const unsigned bands = a.h < 64 ? (unsigned)a.h : 64u;
    hipLaunchKernelGGL(k_u8_max, dim3(bands, (unsigned)n_frames), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_mask_lut, dim3((unsigned)n_frames), dim3(256), 0, s, a);
    const uint32_t groups = (((uint32_t)a.w + 3u) / 4u) * (uint32_t)a.h;
    hipLaunchKernelGGL(k_mask_planar, dim3((groups + 255u) / 256u, (unsigned)n_frames), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_mask_pred_bytes(const MaskPredArgs& a, int n_frames, hipStream_t s)
{
    hipLaunchKernelGGL(k_pred_init, dim3(((unsigned)n_frames + 63u) / 64u), dim3(64), 0, s, a, n_frames);
    const unsigned bands = a.h < 64 ? (unsigned)a.h : 64u;
    hipLaunchKernelGGL(k_pred_minmax, dim3(bands, (unsigned)n_frames), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_pred_bytes, tile_grid(a.w, a.h, n_frames), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdvt
