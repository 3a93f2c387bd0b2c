// mdvt_megasam.hip -- the non-model work of the reference's MegaSAM camera-tracking step (include/mdvt_megasam.h): packed video frames
// to the tracker's planar uint8 image through cv2.resize(INTER_AREA) (mdvt_area_model_frames), depth-coded frames to its float32 depth
// through torch's nearest-exact resize (mdvt_tracker_depth), mask frames to its float32 mask through torch's bilinear resize
// (mdvt_tracker_mask), and its planes out to the packed frames of a depth video and a grey video (mdvt_tracker_outputs).
//
// The unit is compiled with -ffp-contract=off, IEEE division and without fast-math (Makefile): every `*`, `+`, `-` and `/` below is
// one IEEE operation, rounded before the next.  Shared with other units: the four-pixel frame, the plane and pixel stores, cv2's
// linear resize on float32 and the tail of the code kernels (mdvt_depth_code.h); torch's bilinear taps, the two forms of their sum and
// the nearest-exact map (mdvt_torch_resize.h).
//
// k_area_frames: a workgroup per output row of a tile of at most 256 output columns, a frame per blockIdx.z.  The source rows of
// the output row (the vertical taps), over the source columns of the tile, are staged in LDS -- 16 bytes per lane where the layout
// allows, never past the row's own 3 * in_w bytes -- so that a source byte comes from memory once per output row that takes it (a
// row at the border of two output rows twice).  Then a thread per output column and, in turn, channel: the horizontal sum of every
// staged row in ascending tap order, the vertical sum in ascending row order.  The taps of one output are never divided among
// threads: the order of summation is the contract.
//
// k_tracker_depth, k_tracker_mask, k_tracker_codes, k_tracker_grey: a thread per four output pixels of a row, a frame per blockIdx.y.
#include "mdvt_internal.h"
#include "mdvt_device.h"
#include "mdvt_depth_code.h"
#include "mdvt_torch_resize.h"

namespace mdvt {
namespace {

using depth_code::clip_np;
using depth_code::store_plane;
using depth_code::store_pixels;
using depth_code::Quad;
using depth_code::quad_of;
using depth_code::quad_values;
using depth_code::codes_out;
using torch_resize::lin_tap;
using torch_resize::lin_mix;
using torch_resize::nex_idx;

// ---- mdvt_area_model_frames ----------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_area_frames(AreaFramesArgs a)
{
    extern __shared__ uint4 s_rows16[];                             // [rows of the output row][a.lds_row bytes]
    uint8_t* s_rows = reinterpret_cast<uint8_t*>(s_rows16);
    const int y = (int)blockIdx.y;
    const size_t f = (size_t)a.frame0 + blockIdx.z;
    const int x_first = (int)blockIdx.x * a.tile_w;
    const int x_end = x_first + a.tile_w < a.out_w ? x_first + a.tile_w : a.out_w;         // x_first < out_w: the grid has no empty tile
    const int ys = a.y.first[y], yn = a.y.count[y];
    const uint32_t b0 = 3u * (uint32_t)a.x.first[x_first];          // the tile's source bytes of a row: [b0, b1)
    const uint32_t b1 = 3u * (uint32_t)(a.x.first[x_end - 1] + a.x.count[x_end - 1]);
    const uint32_t row_bytes = 3u * (uint32_t)a.in_w;               // b1 <= row_bytes (the table's own check)
    const uint32_t base = a.src_vec ? (b0 & ~15u) : b0;             // LDS byte 0 of a staged row
    const uint8_t* frame = a.src + f * a.src_stride;
    if (a.src_vec) {
        const uint32_t chunks = (b1 - base + 15u) / 16u;            // 16 * chunks <= a.lds_row (the host sized it on the same tables)
        for (uint32_t i = threadIdx.x; i < chunks * (uint32_t)yn; i += 256u) {
            const uint32_t r = i / chunks, ch = i - r * chunks;
            const uint32_t at = base + 16u * ch;
            const uint8_t* src = frame + (size_t)(ys + (int)r) * a.src_pitch + at;
            uint8_t* dst = s_rows + (size_t)r * a.lds_row + 16u * ch;
            if (at + 16u <= row_bytes) {
                *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
            } else {                                                // the row's last bytes: no load passes the row's own end
                for (uint32_t k = 0; at + k < b1; ++k) dst[k] = src[k];
            }
        }
    } else {
        const uint32_t span = b1 - base;
        for (uint32_t i = threadIdx.x; i < span * (uint32_t)yn; i += 256u) {
            const uint32_t r = i / span, k = i - r * span;
            s_rows[(size_t)r * a.lds_row + k] = frame[(size_t)(ys + (int)r) * a.src_pitch + base + k];
        }
    }
    __syncthreads();
    const int x = x_first + (int)threadIdx.x;
    if ((int)threadIdx.x >= a.tile_w || x >= x_end) return;
    const int xn = a.x.count[x];
    const float* alpha = a.x.w + (size_t)x * (size_t)a.x.ktaps;
    const float* beta = a.y.w + (size_t)y * (size_t)a.y.ktaps;
    const uint8_t* taps = s_rows + (3u * (uint32_t)a.x.first[x] - base);
    uint8_t* out = a.dst + f * a.dst_stride + (size_t)y * a.dst_pitch + (size_t)x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                                   // planes R, G, B
        const uint8_t* p = taps + (a.bgr ? 2 - c : c);
        float sum = 0.0f;
        for (int r = 0; r < yn; ++r) {
            float buf = 0.0f;
            for (int k = 0; k < xn; ++k) buf = buf + (float)p[(size_t)r * a.lds_row + 3u * (uint32_t)k] * alpha[k];
            const float t = beta[r] * buf;
            sum = r == 0 ? t : sum + t;
        }
        float v = rintf(sum);                                       // to the nearest, a tie to the even one
        v = v < 0.0f ? 0.0f : v;
        v = v > 255.0f ? 255.0f : v;
        out[(size_t)c * a.dst_plane] = (uint8_t)(int)v;
    }
}

// ---- mdvt_tracker_depth --------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_tracker_depth(TrackerPlaneArgs a)
{
    Quad q;
    if (!quad_of(a.groups, a.gw, a.out_w, a.frame0, q)) return;
    const int sy = nex_idx(q.row, a.scale_y, a.in_h);
    const uint8_t* row = a.src + q.f * a.src_stride + (size_t)sy * a.src_pitch;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < q.nv) {
            const uint32_t px = load_px_bytes(row, nex_idx((uint32_t)(q.x0 + k), a.scale_x, a.in_w));
            const uint32_t red = a.bgr ? (px >> 16) & 0xFFu : px & 0xFFu, blue = a.bgr ? px & 0xFFu : (px >> 16) & 0xFFu;
            d[k] = (float)((red << 24) | (blue << 16)) / a.divisor;            // (16 significant bits: the conversion is exact)
        }
    }
    store_plane(reinterpret_cast<float*>(a.dst + q.f * a.dst_stride + (size_t)q.row * a.dst_pitch) + q.x0, d, q.nv, a.dst_vec != 0);
}

// ---- mdvt_tracker_mask ---------------------------------------------------------------------------------------------------------

// 255 - OpenCV's 8-bit grey of a packed pixel
__device__ __forceinline__ uint32_t inverted_grey(uint32_t px, int bgr)
{
    const uint32_t c0 = px & 0xFFu, g = (px >> 8) & 0xFFu, c2 = (px >> 16) & 0xFFu;
    const uint32_t r = bgr ? c2 : c0, b = bgr ? c0 : c2;
    return 255u - ((4899u * r + 9617u * g + 1868u * b + 8192u) >> 14);
}

__global__ void __launch_bounds__(256) k_tracker_mask(TrackerPlaneArgs a)
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
    float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < q.nv) {
            int x0, x1;
            float wx0, wx1;
            lin_tap(q.x0 + k, a.scale_x, a.in_w, x0, x1, wx0, wx1);
            const float v00 = s_unit[inverted_grey(load_px_bytes(r0, x0), a.bgr)], v01 = s_unit[inverted_grey(load_px_bytes(r0, x1), a.bgr)];
            const float v10 = s_unit[inverted_grey(load_px_bytes(r1, x0), a.bgr)], v11 = s_unit[inverted_grey(load_px_bytes(r1, x1), a.bgr)];
            d[k] = lin_mix(a.small != 0, wy0, wy1, wx0, wx1, v00, v01, v10, v11);
        }
    }
    store_plane(reinterpret_cast<float*>(a.dst + q.f * a.dst_stride + (size_t)q.row * a.dst_pitch) + q.x0, d, q.nv, a.dst_vec != 0);
}

// ---- mdvt_tracker_outputs ------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_tracker_codes(TrackerOutArgs a)
{
    Quad q;
    if (!quad_of(a.c.groups, a.c.gw, a.c.out_w, a.c.frame0, q)) return;
    const int sy = nex_idx(q.row, a.scale_y, a.c.in_h);
    const float* row = reinterpret_cast<const float*>(a.c.src + q.f * a.c.src_stride + (size_t)sy * a.c.src_pitch);
    float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < q.nv) d[k] = row[nex_idx((uint32_t)(q.x0 + k), a.scale_x, a.c.in_w)];
    codes_out(d, q, a.c);
}

template <bool RESIZE>
__global__ void __launch_bounds__(256) k_tracker_grey(TrackerOutArgs a)
{
    Quad q;
    if (!quad_of(a.c.groups, a.c.gw, a.c.out_w, a.c.frame0, q)) return;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    quad_values(d, a.c.src + q.f * a.c.src_stride, a.c.src_pitch, a.c.src_vec != 0, q, RESIZE, a.c.ratio_x, a.c.ratio_y, a.c.in_w, a.c.in_h,
                [](float x) { return x; });
    const float m = a.c.fmax;
    uint32_t px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float g = clip_np(d[k], m) / m * 255.0f;
        const uint32_t b = (g >= 0.0f && g < 256.0f) ? (uint32_t)g : 0u;        // truncation; a NaN gives 0 (the header's decree)
        px[k] = b | (b << 8) | (b << 16);
    }
    store_pixels(a.c.codes + q.f * a.c.codes_stride + (size_t)q.row * a.c.codes_pitch + (size_t)q.x0 * 3u, px, q.nv, a.c.codes_vec != 0);
}

}  // namespace

hipError_t launch_area_frames(const AreaFramesArgs& a, int n_frames, hipStream_t s)
{
    const dim3 grid(((unsigned)a.out_w + (unsigned)a.tile_w - 1u) / (unsigned)a.tile_w, (unsigned)a.out_h, (unsigned)n_frames);
    hipLaunchKernelGGL(k_area_frames, grid, dim3(256), (size_t)a.y.ktaps * a.lds_row, s, a);
    return hipGetLastError();
}

hipError_t launch_tracker_depth(const TrackerPlaneArgs& a, int n_frames, hipStream_t s)
{
    const dim3 grid((a.groups + 255u) / 256u, (unsigned)n_frames);
    hipLaunchKernelGGL(k_tracker_depth, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tracker_mask(const TrackerPlaneArgs& a, int n_frames, hipStream_t s)
{
    const dim3 grid((a.groups + 255u) / 256u, (unsigned)n_frames);
    hipLaunchKernelGGL(k_tracker_mask, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tracker_codes(const TrackerOutArgs& a, int n_frames, hipStream_t s)
{
    const dim3 grid((a.c.groups + 255u) / 256u, (unsigned)n_frames);
    hipLaunchKernelGGL(k_tracker_codes, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tracker_grey(const TrackerOutArgs& a, int n_frames, hipStream_t s)
{
    const dim3 grid((a.c.groups + 255u) / 256u, (unsigned)n_frames);
    if (a.c.resize) hipLaunchKernelGGL(k_tracker_grey<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_tracker_grey<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdvt
