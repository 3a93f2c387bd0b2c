// mdvt_formats.hip -- the streaming kernels around the render that depend neither on the sub-pixel grid nor on a tuning hook:
// the depth codec (dfh), k_zero_bytes, the Touchly inverse-depth plane, the VR180 equirectangular remap and the R <-> B swap, with
// their launchers.  Compiled once and linked into both libraries.
//
// Compiled with -ffp-contract=off: see the arithmetic decree in mdvt_device.h / DESIGN.md.
#include "mdvt_device.h"

namespace mdvt {

// =================================================================================================
// depth codec (dfh)
// =================================================================================================

__global__ void k_decode_depth(const uint8_t* __restrict__ rgb, size_t rgb_pitch, float* __restrict__ out,
                               size_t out_pitch, int W, int H, float mult, float scale)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= W || i >= H) return;
    const uint32_t px = load_px_bytes(rgb + (size_t)i * rgb_pitch, j);
    float* orow = (float*)((uint8_t*)out + (size_t)i * out_pitch);
    orow[j] = decode_z(code16_of(px), mult, scale);
}

// 4 pixels per thread: 12 B coalesced load, 16 B coalesced store.
__global__ void k_decode_depth4(const uint8_t* __restrict__ rgb, size_t rgb_pitch, float* __restrict__ out,
                                size_t out_pitch, int W4, int H, float mult, float scale)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (g >= W4 || i >= H) return;
    const uint32_t* src = (const uint32_t*)(rgb + (size_t)i * rgb_pitch) + 3 * (size_t)g;
    uint32_t px[4];
    unpack4(src[0], src[1], src[2], px);
    float4 z;
    z.x = decode_z(code16_of(px[0]), mult, scale);
    z.y = decode_z(code16_of(px[1]), mult, scale);
    z.z = decode_z(code16_of(px[2]), mult, scale);
    z.w = decode_z(code16_of(px[3]), mult, scale);
    ((float4*)((uint8_t*)out + (size_t)i * out_pitch))[g] = z;
}

hipError_t launch_decode_depth(const uint8_t* rgb, size_t rgb_pitch, float* out, size_t out_pitch, int W, int H,
                               float mult, float scale, hipStream_t s)
{
    const bool vec = (W % 4 == 0) && (rgb_pitch % 4 == 0) && (out_pitch % 16 == 0) &&
                     ((uintptr_t)rgb % 4 == 0) && ((uintptr_t)out % 16 == 0);
    if (vec) {
        const int W4 = W / 4;
        dim3 grid((W4 + 255) / 256, H);
        hipLaunchKernelGGL(k_decode_depth4, grid, dim3(256), 0, s, rgb, rgb_pitch, out, out_pitch, W4, H, mult, scale);
    } else {
        dim3 grid((W + 255) / 256, H);
        hipLaunchKernelGGL(k_decode_depth, grid, dim3(256), 0, s, rgb, rgb_pitch, out, out_pitch, W, H, mult, scale);
    }
    return hipGetLastError();
}

// dfh:5-11: clip to [0,max] in f32, f64 multiply by 255^4/max, truncate to u32; dfh:53-55: R = G = byte 3,
// B = byte 2.
__global__ void k_encode_depth(const float* __restrict__ depth, size_t depth_pitch, uint8_t* __restrict__ rgb,
                               size_t rgb_pitch, int W, int H, double multi, float fmax_depth, int bgr)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= W || i >= H) return;
    float d = ((const float*)((const uint8_t*)depth + (size_t)i * depth_pitch))[j];
    if (d > fmax_depth) d = fmax_depth;
    if (d < 0.0f) d = 0.0f;
    const double e = multi * (double)d;
    const uint32_t code = (e >= 0.0 && e < 4294967296.0) ? (uint32_t)e : 0u;     // NaN -> 0
    const uint32_t hi = code >> 24, lo = (code >> 16) & 0xFFu;
    const uint32_t px = bgr ? (lo | (hi << 8) | (hi << 16)) : (hi | (hi << 8) | (lo << 16));
    store_px_bytes(rgb + (size_t)i * rgb_pitch, j, px);
}

hipError_t launch_encode_depth(const float* depth, size_t depth_pitch, uint8_t* rgb, size_t rgb_pitch, int W, int H,
                               double max_depth, int bgr, hipStream_t s)
{
    dim3 grid((W + 255) / 256, H);
    hipLaunchKernelGGL(k_encode_depth, grid, dim3(256), 0, s, depth, depth_pitch, rgb, rgb_pitch, W, H,
                       4228250625.0 / max_depth, (float)max_depth, bgr);
    return hipGetLastError();
}

// Zero `bytes` bytes at `p` (any alignment): 16-byte stores over the aligned body, byte stores at its two ends.  Replaces the per-set
// hipMemsetAsync of the 89-degree filter's flag plane (two runtime fill launches, 13 us per 16 MB): one launch; measured, a single
// product-default frame per call 148.9 -> 146.7 us, 32 frames per call unchanged (the fills hid behind the other bank's walk).
__global__ void __launch_bounds__(256) k_zero_bytes(uint8_t* p, size_t bytes)
{
    const size_t head = min(bytes, (size_t)((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u));
    const size_t body = (bytes - head) >> 4, tail0 = head + (body << 4);
    uint4* q = reinterpret_cast<uint4*>(p + head);
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x, nt = (size_t)gridDim.x * 256u;
    for (size_t k = t; k < body; k += nt) q[k] = make_uint4(0u, 0u, 0u, 0u);
    if (t < head) p[t] = 0;
    if (t < bytes - tail0) p[tail0 + t] = 0;
}
hipError_t launch_zero_bytes(void* p, size_t bytes, hipStream_t s)
{
    if (!bytes) return hipSuccess;
    const size_t blocks = (bytes / 16 + 255) / 256;
    hipLaunchKernelGGL(k_zero_bytes, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks))), dim3(256), 0, s, (uint8_t*)p, bytes);
    return hipGetLastError();
}

// Touchly inverse-depth plane (sr:549-551, 689-691, 825-829).
__global__ void __launch_bounds__(256) k_touchly_depth(const float* __restrict__ depth, size_t depth_pitch,
                                                       uint8_t* __restrict__ rgb, size_t rgb_pitch, int W, int H,
                                                       float tmax, float tmin, float k, int zero_is_far)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= W) return;
    const float d = ((const float*)((const uint8_t*)depth + (size_t)y * depth_pitch))[x];
    const float v = rintf(fmaxf(0.0f, fminf(d, tmax) - tmin) * k);
    uint32_t q = (uint32_t)v & 0xFFu;                       // .astype(np.uint8)
    if (zero_is_far && q == 0) q = 255;                     // sr:690 / 827
    q = 255u - q;                                           // Touchly uses reverse depth
    store_px_bytes(rgb + (size_t)y * rgb_pitch, x, q | (q << 8) | (q << 16));
}

hipError_t launch_touchly_depth(const float* depth, size_t depth_pitch, uint8_t* rgb, size_t rgb_pitch, int W, int H,
                                float tmax, float tmin, float k, int zero_is_far, hipStream_t s)
{
    dim3 grid((W + 255) / 256, H);
    hipLaunchKernelGGL(k_touchly_depth, grid, dim3(256), 0, s, depth, depth_pitch, rgb, rgb_pitch, W, H, tmax, tmin, k, zero_is_far);
    return hipGetLastError();
}

// =================================================================================================
// VR180: convert_to_equirectangular (sr:25-86) = cv2.remap(INTER_LINEAR, BORDER_CONSTANT 0) through
// separable lookup tables
// =================================================================================================
// One thread = PX output pixels of one row of one image.  Coordinates are rounded to 1/32 px (half to even),
// the four taps get the integer weights (32-fx)(32-fy)*32 ... (sum 2^15), taps outside the image are 0, the
// result is (sum + 2^14) >> 15.  A table entry of -1 marks an angle outside the input fov: the pixel is black.
__device__ __forceinline__ uint32_t remap_tap4(const uint8_t* __restrict__ src, size_t pitch, int W, int H,
                                               int ix, int iy, int fx, int fy)
{
    const int w00 = (32 - fx) * (32 - fy) * 32, w10 = fx * (32 - fy) * 32, w01 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
    const bool x0 = ix >= 0 && ix < W, x1 = ix + 1 >= 0 && ix + 1 < W;
    const bool y0 = iy >= 0 && iy < H, y1 = iy + 1 >= 0 && iy + 1 < H;
    const uint32_t p00 = (x0 && y0) ? load_px_bytes(src + (size_t)iy * pitch, ix) : 0u;
    const uint32_t p10 = (x1 && y0 && w10) ? load_px_bytes(src + (size_t)iy * pitch, ix + 1) : 0u;
    const uint32_t p01 = (x0 && y1 && w01) ? load_px_bytes(src + (size_t)(iy + 1) * pitch, ix) : 0u;
    const uint32_t p11 = (x1 && y1 && w11) ? load_px_bytes(src + (size_t)(iy + 1) * pitch, ix + 1) : 0u;
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int sh = 8 * c;
        const int acc = w00 * (int)((p00 >> sh) & 0xFF) + w10 * (int)((p10 >> sh) & 0xFF) +
                        w01 * (int)((p01 >> sh) & 0xFF) + w11 * (int)((p11 >> sh) & 0xFF);
        out |= (uint32_t)((acc + (1 << 14)) >> 15) << sh;
    }
    return out;
}

template <int PX>
__global__ void __launch_bounds__(256) k_equirect_remap(const uint8_t* __restrict__ src, size_t src_pitch, size_t src_stride,
                                                        uint8_t* __restrict__ dst, size_t dst_pitch, size_t dst_stride,
                                                        int W, int H, const float* __restrict__ mx, const float* __restrict__ my)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (g >= W / PX) return;
    const uint8_t* simg = src + (size_t)blockIdx.z * src_stride;
    uint8_t* drow = dst + (size_t)blockIdx.z * dst_stride + (size_t)y * dst_pitch;
    const float fyv = my[y];
    uint32_t out[PX];
    if (fyv == -1.0f) {
#pragma unroll
        for (int q = 0; q < PX; ++q) out[q] = 0u;
    } else {
        const int sy = (int)rintf(fyv * 32.0f);
#pragma unroll
        for (int q = 0; q < PX; ++q) {
            const float fxv = mx[g * PX + q];
            if (fxv == -1.0f) { out[q] = 0u; continue; }
            const int sx = (int)rintf(fxv * 32.0f);
            out[q] = remap_tap4(simg, src_pitch, W, H, sx >> 5, sy >> 5, sx & 31, sy & 31);
        }
    }
    RowIO<PX>::store_rgb(drow, g, out);
}

hipError_t launch_equirect_remap(const uint8_t* src, size_t src_pitch, size_t src_stride, uint8_t* dst, size_t dst_pitch,
                                 size_t dst_stride, int n, int W, int H, const float* mx, const float* my, hipStream_t s)
{
    const bool vec4 = W % 4 == 0 && ((uintptr_t)dst % 4 == 0) && dst_pitch % 4 == 0 && dst_stride % 4 == 0;
    if (vec4) {
        dim3 grid((W / 4 + 255) / 256, H, n);
        hipLaunchKernelGGL((k_equirect_remap<4>), grid, dim3(256), 0, s, src, src_pitch, src_stride, dst, dst_pitch, dst_stride, W, H, mx, my);
    } else {
        dim3 grid((W + 255) / 256, H, n);
        hipLaunchKernelGGL((k_equirect_remap<1>), grid, dim3(256), 0, s, src, src_pitch, src_stride, dst, dst_pitch, dst_stride, W, H, mx, my);
    }
    return hipGetLastError();
}

// cv2.cvtColor(BGR2RGB / RGB2BGR) of interleaved u8 frames (sr:493, 505, 928, 941): bytes 0 and 2 of every pixel swap.
template <int PX>
__global__ void __launch_bounds__(256) k_swap_rb(ImageSet src, ImageSet dst, int W, int H)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, im = blockIdx.z;
    if (g >= W / PX) return;
    uint32_t px[PX];
    RowIO<PX>::load_nt(src.image(im) + (size_t)y * src.pitch, g, px);
#pragma unroll
    for (int q = 0; q < PX; ++q) px[q] = (px[q] & 0x00FF00u) | ((px[q] >> 16) & 0xFFu) | ((px[q] & 0xFFu) << 16);
    RowIO<PX>::store_rgb(dst.image(im) + (size_t)y * dst.pitch, g, px);
}

hipError_t launch_swap_rb(const ImageSet& src, const ImageSet& dst, int n, int W, int H, hipStream_t s)
{
    const bool vec4 = W % 4 == 0 && ((uintptr_t)src.base % 4 == 0) && ((uintptr_t)dst.base % 4 == 0) && src.pitch % 4 == 0 &&
                      dst.pitch % 4 == 0 && src.stride % 4 == 0 && dst.stride % 4 == 0;
    if (vec4) hipLaunchKernelGGL((k_swap_rb<4>), dim3((W / 4 + 255) / 256, H, n), dim3(256), 0, s, src, dst, W, H);
    else hipLaunchKernelGGL((k_swap_rb<1>), dim3((W + 255) / 256, H, n), dim3(256), 0, s, src, dst, W, H);
    return hipGetLastError();
}

}  // namespace mdvt
