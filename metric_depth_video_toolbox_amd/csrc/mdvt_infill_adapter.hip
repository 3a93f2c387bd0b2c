// mdvt_infill_adapter.hip -- the device side of the StereoCrafter infill step around its model (include/mdvt_infill_adapter.h):
// the reference's per-frame host code of stereo_crafter_infill.py ("scr") and infill_common.py ("ic").
//
//   k_adapter_prepare     scr:101-126  an eye of the side-by-side colour and mask frames -> the model's image and mask (the u8 resize
//                                      restated in the header; the left eye read mirrored) and the holes of each model mask
//   k_lhm_moments         ic:98-118    count, sums and second moments of a frame's pixels as exact integers: a lane sums at most
//                                      kMomentsWiden pixels in 32 bits, then widens; waves join by shuffles, workgroups by 64-bit
//                                      integer atomics (exact, so the launch geometry cannot show in the result)
//   k_lhm_apply           ic:126-128   y = A (x - mu_x) + mu_r in float64, every product and sum rounded
//   k_adapter_hblur,      scr:151-188  the 15-tap Gaussian of the grown lower-side marks (rows, then columns, in k_adapter_composite),
//   k_adapter_composite                the model frame resized back, pasted under the mask and blended by that alpha
// The lower-side marks and their six cross dilations come from mdvt_normal_infill.hip (launch_mark_lower_side, launch_grow_marks); the u8
// resize is mdvt_adapter_resize.h's.
//
// The unit is compiled with -ffp-contract=off and without fast-math (Makefile): every `*`, `+` and `-` below is one IEEE operation.
#include "mdvt_device.h"
#include "mdvt_adapter_resize.h"

namespace mdvt {
namespace {

// scr:101-126.  A thread per model pixel; grid (columns / 256, rows, frames).
__global__ void __launch_bounds__(256) k_adapter_prepare(AdapterPrepareArgs a)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const size_t f = blockIdx.z;
    bool hole = false;
    if (x < a.rs.out_w) {
        const uint8_t* color = a.color.p + f * a.color.stride;
        const uint8_t* mask = a.mask.p + f * a.mask.stride;
        const int last = a.rs.in_w - 1, mirror = a.mirror;
        const uint32_t c = adapter_resize_px(a.rs, x, y, [&](int sx, int sy) {
            return load_px_bytes(color + (size_t)sy * a.color.pitch, mirror ? last - sx : sx);
        });
        const uint32_t m = adapter_resize_px(a.rs, x, y, [&](int sx, int sy) {
            return load_px_bytes(mask + (size_t)sy * a.mask.pitch, mirror ? last - sx : sx) != 0u ? 255u : 0u;      // scr:104, 117
        });
        hole = m != 0u;                                                                                            // scr:106, 119: > 0
        store_px_bytes(a.image + f * a.image_stride + (size_t)y * a.image_pitch, x, c);
        a.mmask[f * a.mmask_stride + (size_t)y * a.mmask_pitch + x] = hole ? 255 : 0;
    }
    const unsigned long long b = __ballot(hole);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(a.holes + f, (uint32_t)__popcll(b));
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// ic:98-118.  Grid (workgroups, frames); workgroup b takes the rows b, b + gridDim.x, ..., a thread four pixels of a row at a time
// (VEC: as three dwords) or one.
template <int VEC>
__global__ void __launch_bounds__(256) k_lhm_moments(LhmMomentsArgs a)
{
    constexpr int PX = VEC ? 4 : 1;
    __shared__ unsigned long long s_part[4][10];
    const size_t f = blockIdx.y;
    const uint8_t* img = a.img.p + f * a.img.stride;
    const uint8_t* mask = a.mask.p ? a.mask.p + f * a.mask.stride : nullptr;
    unsigned long long wide[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, held = 0;     // held: pixels the 32-bit sums may hold
    const int groups = (a.W + PX - 1) / PX;
    for (int y = blockIdx.x; y < a.H; y += gridDim.x) {
        const uint8_t* row = img + (size_t)y * a.img.pitch;
        const uint8_t* mrow = mask ? mask + (size_t)y * a.mask.pitch : nullptr;
        for (int g = threadIdx.x; g < groups; g += 256) {
            if (held + PX > kMomentsWiden) {                         // the bound: at most kMomentsWiden pixels between two widenings
#pragma unroll
                for (int k = 0; k < 10; ++k) { wide[k] += acc[k]; acc[k] = 0; }
                held = 0;
            }
            held += PX;
            uint32_t px[PX], skip[PX];
            const int x0 = g * PX, nv = a.W - x0 < PX ? a.W - x0 : PX;
            if (VEC && nv == 4) {
                uint32_t p4[4];
                RowIO<4>::load(row, g, p4);
                const uint32_t m4 = mrow ? *reinterpret_cast<const uint32_t*>(mrow + x0) : 0u;
#pragma unroll
                for (int q = 0; q < PX; ++q) { px[q] = p4[q]; skip[q] = (m4 >> (8 * q)) & 0xFFu; }
            } else {
#pragma unroll
                for (int q = 0; q < PX; ++q) {
                    px[q] = q < nv ? load_px_bytes(row, x0 + q) : 0u;
                    skip[q] = q < nv ? (mrow ? mrow[x0 + q] : 0u) : 1u;
                }
            }
#pragma unroll
            for (int q = 0; q < PX; ++q) {
                if (skip[q]) continue;
                const uint32_t r = px[q] & 0xFFu, gg = (px[q] >> 8) & 0xFFu, b = px[q] >> 16;
                acc[0] += 1u; acc[1] += r; acc[2] += gg; acc[3] += b;
                acc[4] += r * r; acc[5] += r * gg; acc[6] += r * b; acc[7] += gg * gg; acc[8] += gg * b; acc[9] += b * b;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const unsigned long long v = wave_sum(wide[k] + acc[k]);
        if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 10) {
        const unsigned long long v = (s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + (s_part[2][threadIdx.x] + s_part[3][threadIdx.x]);
        if (v) atomicAdd(a.out + f * 10 + threadIdx.x, v);
    }
}

// ic:102, 126-128.  A thread per four pixels of a row (VEC: three dwords in, three out) or per pixel; grid (groups / 256, rows, frames).
template <int VEC>
__global__ void __launch_bounds__(256) k_lhm_apply(LhmApplyArgs a)
{
    constexpr int PX = VEC ? 4 : 1;
    const int g = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, x0 = g * PX;
    const size_t f = blockIdx.z;
    if (x0 >= a.W) return;
    const double* P = a.params + f * 15;
    double A[9], mx[3], mr[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) A[k] = P[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) { mx[k] = P[9 + k]; mr[k] = P[12 + k]; }
    const uint8_t* row = a.img.p + f * a.img.stride + (size_t)y * a.img.pitch;
    uint8_t* orow = a.out + f * a.out_stride + (size_t)y * a.out_pitch;
    const int nv = a.W - x0 < PX ? a.W - x0 : PX;
    uint32_t px[PX];
    if (VEC && nv == 4) {
        uint32_t p4[4];
        RowIO<4>::load(row, g, p4);
#pragma unroll
        for (int q = 0; q < PX; ++q) px[q] = p4[q];
    } else {
#pragma unroll
        for (int q = 0; q < PX; ++q) px[q] = q < nv ? load_px_bytes(row, x0 + q) : 0u;
    }
#pragma unroll
    for (int q = 0; q < PX; ++q) {
        const double d0 = (double)(px[q] & 0xFFu) - mx[0], d1 = (double)((px[q] >> 8) & 0xFFu) - mx[1], d2 = (double)(px[q] >> 16) - mx[2];
        uint32_t o = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double yv = ((d0 * A[3 * c] + d1 * A[3 * c + 1]) + d2 * A[3 * c + 2]) + mr[c];
            const double r = rint(yv);                                // np.round: half to even
            o |= (r >= 255.0 ? 255u : r > 0.0 ? (uint32_t)r : 0u) << (8 * c);
        }
        px[q] = o;
    }
    if (VEC && nv == 4) {
        uint32_t p4[4] = {px[0], px[PX > 1 ? 1 : 0], px[PX > 2 ? 2 : 0], px[PX > 3 ? 3 : 0]}, w0, w1, w2;
        pack4(p4, w0, w1, w2);
        uint32_t* op = reinterpret_cast<uint32_t*>(orow) + 3 * (size_t)g;
        op[0] = w0; op[1] = w1; op[2] = w2;
    } else {
#pragma unroll
        for (int q = 0; q < PX; ++q)
            if (q < nv) store_px_bytes(orow, x0 + q, px[q]);
    }
}

__device__ __forceinline__ int adapter_reflect101(int p, int len) { return p < 0 ? -p : p >= len ? 2 * len - 2 - p : p; }      // len >= 8, |taps| <= 7

// The Gaussian's horizontal pass over the 0 / 1 plane: a 15-term sum from the left, every product and sum rounded.
__global__ void __launch_bounds__(256) k_adapter_hblur(AdapterCompositeArgs a)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, W = a.rs.out_w;
    if (x >= W) return;
    const uint8_t* row = a.grown + (size_t)y * W;
    float acc = a.g.w[0] * (float)row[adapter_reflect101(x - 7, W)];
#pragma unroll
    for (int i = 1; i < 15; ++i) acc = acc + a.g.w[i] * (float)row[adapter_reflect101(x + i - 7, W)];
    a.hblur[(size_t)y * W + x] = acc;
}

// scr:152-188 for one pixel of the eye: the vertical pass gives alpha; the model pixel is fetched only where it shows (under the
// mask or where alpha is not 0: with alpha 0 the blend is fl(0 * m) + fl(1 * p) = p whatever m is).
__global__ void __launch_bounds__(256) k_adapter_composite(AdapterCompositeArgs a)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, W = a.rs.out_w, H = a.rs.out_h;
    if (x >= W) return;
    float alpha = a.g.w[0] * a.hblur[(size_t)adapter_reflect101(y - 7, H) * W + x];
#pragma unroll
    for (int i = 1; i < 15; ++i) alpha = alpha + a.g.w[i] * a.hblur[(size_t)adapter_reflect101(y + i - 7, H) * W + x];
    const uint32_t org = load_px_bytes(a.color.p + (size_t)y * a.color.pitch, x);
    const bool under = load_px_bytes(a.mask.p + (size_t)y * a.mask.pitch, x) != 0u;        // scr:161-165
    uint32_t pasted = org, blended = org;
    if (under || alpha != 0.0f) {
        const int last = a.rs.in_w - 1, mirror = a.mirror;
        const uint8_t* model = a.model.p;
        const size_t pitch = a.model.pitch;
        const uint32_t m = adapter_resize_px(a.rs, x, y, [&](int sx, int sy) {
            return load_px_bytes(model + (size_t)sy * pitch, mirror ? last - sx : sx);     // scr:152: the left eye's frame flipped back
        });
        if (under) pasted = m;
        blended = 0;
        const float rest = 1.0f - alpha;
#pragma unroll
        for (int k = 0; k < 24; k += 8) {
            const float v = alpha * (float)((m >> k) & 0xFFu) + rest * (float)((pasted >> k) & 0xFFu);           // scr:183-184
            blended |= (v >= 255.0f ? 255u : v > 0.0f ? (uint32_t)v : 0u) << k;                                  // scr:187: clip, truncate
        }
    }
    store_px_bytes(a.pasted + (size_t)y * a.pasted_pitch, x, pasted);
    store_px_bytes(a.blended + (size_t)y * a.blended_pitch, x, blended);
}

}  // namespace

AdapterResize adapter_resize(int in_w, int in_h, int out_w, int out_h)
{
    AdapterResize r{};
    r.in_w = in_w; r.in_h = in_h; r.out_w = out_w; r.out_h = out_h;
    r.mode = (in_w == out_w && in_h == out_h) ? 0 : (in_w == 2 * out_w && in_h == 2 * out_h) ? 1 : 2;
    r.rx = (double)in_w / (double)out_w; r.ry = (double)in_h / (double)out_h;
    return r;
}

hipError_t launch_adapter_prepare(const AdapterPrepareArgs& a, int n, hipStream_t s)
{
    hipLaunchKernelGGL(k_adapter_prepare, dim3((a.rs.out_w + 255) / 256, a.rs.out_h, n), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_lhm_moments(const LhmMomentsArgs& a, int n, hipStream_t s)
{
    const dim3 grid(a.H < 256 ? a.H : 256, n);
    if (a.vec) hipLaunchKernelGGL(k_lhm_moments<1>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_lhm_moments<0>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_lhm_apply(const LhmApplyArgs& a, int n, hipStream_t s)
{
    const int groups = a.vec ? (a.W + 3) / 4 : a.W;
    const dim3 grid((groups + 255) / 256, a.H, n);
    if (a.vec) hipLaunchKernelGGL(k_lhm_apply<1>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_lhm_apply<0>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_adapter_composite(const AdapterCompositeArgs& a, hipStream_t s)
{
    const dim3 grid((a.rs.out_w + 255) / 256, a.rs.out_h);
    hipLaunchKernelGGL(k_adapter_hblur, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_adapter_composite, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdvt
