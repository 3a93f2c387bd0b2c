// mdvt_edge_filter.hip -- the 89-degree oblique-triangle filter of the mesh (dmt:1283-1294, 1339-1344): k_edge_filter[4] and
// launch_edge_filter.  Depends neither on the sub-pixel grid nor on a tuning hook: compiled once and linked into both libraries.
//
// Compiled with -ffp-contract=off: see the arithmetic decree in mdvt_device.h / DESIGN.md.
#include "mdvt_edge_filter.h"

namespace mdvt {

__device__ __forceinline__ void edge_filter_mark_unused(uint8_t* u, int W, int i, int j, uint32_t inv)
{
    const size_t a = (size_t)i * W + j;
    u[a] = 1;                          // A
    u[a + W + 1] = 1;                  // C
    if (inv & 1u) u[a + W] = 1;        // B
    if (inv & 2u) u[a + 1] = 1;        // D
}

// One thread per grid cell: both triangles of the cell.  `unused` must be zeroed beforehand.  (Any width / alignment.)
// NOTE f.sx / f.sy hold the mesh grid scale only when the frame was prepared for mesh mode; the host
// passes scale factors explicitly so the filter can be run standalone for either grid.
__global__ void __launch_bounds__(128) k_edge_filter(const uint8_t* __restrict__ depth_rgb, size_t pitch, size_t stride,
                              const FrameDev* __restrict__ fp, int frame0, int W, int H, int of_by_one,
                              float sx, float sy,
                              uint8_t* __restrict__ tri_invalid, size_t tri_stride,
                              uint8_t* __restrict__ unused, size_t unused_stride)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    const int fr = blockIdx.z;
    if (j >= W - 1 || i >= H - 1) return;
    const uint8_t* r0 = depth_rgb + (size_t)(frame0 + fr) * stride + (size_t)i * pitch;
    const uint8_t* r1 = r0 + pitch;
    const uint32_t pA = load_px_bytes(r0, j), pD = load_px_bytes(r0, j + 1);
    const uint32_t pB = load_px_bytes(r1, j), pC = load_px_bytes(r1, j + 1);
    FrameDev f = fp[frame0 + fr];
    f.sx = sx; f.sy = sy;
    const float zA = decode_z(code16_of(pA), f.mult, f.scale);
    const float zD = decode_z(code16_of(pD), f.mult, f.scale);
    const float zB = decode_z(code16_of(pB), f.mult, f.scale);
    const float zC = decode_z(code16_of(pC), f.mult, f.scale);
    // screening vertices: the same unprojection with a reciprocal instead of the two divisions
    const double rfx = f.rKd[0], rfy = f.rKd[1];
    const double x0 = (of_by_one ? (double)((float)j * f.sx) : (double)j) - f.Kd[2];
    const double x1 = (of_by_one ? (double)((float)(j + 1) * f.sx) : (double)(j + 1)) - f.Kd[2];
    const double y0 = (of_by_one ? (double)((float)i * f.sy) : (double)i) - f.Kd[3];
    const double y1 = (of_by_one ? (double)((float)(i + 1) * f.sy) : (double)(i + 1)) - f.Kd[3];
    const double x0r = x0 * rfx, x1r = x1 * rfx, y0r = y0 * rfy, y1r = y1 * rfy;
    const uint32_t inv = edge_filter_cell(f, i, j, of_by_one, x0r, x1r, y0r, y1r, edge_filter_prescreen(cell_rays_f32(x0r, x1r, y0r, y1r), zA, zB, zC, zD), zA, zB, zC, zD);
    const size_t ncell = (size_t)(W - 1) * (H - 1);
    const size_t cell = (size_t)i * (W - 1) + j;
    if (tri_invalid) {
        uint8_t* t = tri_invalid + (size_t)fr * tri_stride;
        t[cell] = inv & 1u;
        t[ncell + cell] = (inv >> 1) & 1u;
    }
    if (unused && inv) edge_filter_mark_unused(unused + (size_t)fr * unused_stride, W, i, j, inv);
}

// The same for dword-addressable rows (W % 4 == 0, 4-byte aligned base / pitch / stride): a thread takes FOUR cells of a
// row -- five pixels of two rows as 2 x 4 dwords instead of 2 x 10 byte loads, the eight validity bytes as two dword stores.
// (r04: with the f32 pre-screen no f64 instruction runs on ordinary content, and the one-cell kernel turned out to be bound
// by its byte accesses, not by the f64 rate its design assumed: 10.4 -> see DESIGN.md us per 1080p frame.)
typedef uint32_t u32_unaligned_t __attribute__((aligned(1)));
__global__ void __launch_bounds__(128) k_edge_filter4(const uint8_t* __restrict__ depth_rgb, size_t pitch, size_t stride,
                              const FrameDev* __restrict__ fp, int frame0, int W, int H, int of_by_one,
                              float sx, float sy,
                              uint8_t* __restrict__ tri_invalid, size_t tri_stride,
                              uint8_t* __restrict__ unused, size_t unused_stride)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    const int fr = blockIdx.z;
    const int j0 = 4 * g;
    if (j0 >= W - 1 || i >= H - 1) return;
    const uint32_t* r0 = (const uint32_t*)(depth_rgb + (size_t)(frame0 + fr) * stride + (size_t)i * pitch) + 3 * g;
    const uint32_t* r1 = (const uint32_t*)((const uint8_t*)r0 + pitch);
    const bool five = j0 + 4 < W;                          // (the last group of a row has no fifth pixel -- and no fourth cell)
    uint32_t p0[5], p1[5];
    unpack4(r0[0], r0[1], r0[2], *(uint32_t(*)[4])p0);
    unpack4(r1[0], r1[1], r1[2], *(uint32_t(*)[4])p1);
    p0[4] = five ? r0[3] & 0xFFFFFFu : 0u;
    p1[4] = five ? r1[3] & 0xFFFFFFu : 0u;
    FrameDev f = fp[frame0 + fr];
    f.sx = sx; f.sy = sy;
    float z0[5], z1[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        z0[q] = decode_z(code16_of(p0[q]), f.mult, f.scale);
        z1[q] = decode_z(code16_of(p1[q]), f.mult, f.scale);
    }
    const double rfx = f.rKd[0], rfy = f.rKd[1];
    const double y0r = ((of_by_one ? (double)((float)i * f.sy) : (double)i) - f.Kd[3]) * rfy;
    const double y1r = ((of_by_one ? (double)((float)(i + 1) * f.sy) : (double)(i + 1)) - f.Kd[3]) * rfy;
    double xr[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) xr[q] = ((of_by_one ? (double)((float)(j0 + q) * f.sx) : (double)(j0 + q)) - f.Kd[2]) * rfx;
    const int ncells = five ? 4 : 3;
    float fx[5];
    const float fb = (float)y0r, fb1 = (float)y1r, fpy = (float)(y1r - y0r);
    bool rays_ok = fabsf(fb) <= 64.0f && fabsf(fb1) <= 64.0f;
#pragma unroll
    for (int q = 0; q < 5; ++q) { fx[q] = (float)xr[q]; rays_ok = rays_ok && fabsf(fx[q]) <= 64.0f; }
    uint32_t w1 = 0, w2 = 0, any = 0;
    uint32_t inv[4] = {0, 0, 0, 0}, pre[4] = {0, 0, 0, 0};
    // all eight triangles through the f32 pre-screen first (straight-line code); the f64 paths behind ONE branch
    uint32_t und = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < ncells) {
            CellRaysF32 r;
            r.a = fx[q]; r.a1 = fx[q + 1]; r.b = fb; r.b1 = fb1; r.px = (float)(xr[q + 1] - xr[q]); r.py = fpy;
            r.ok = rays_ok;
            pre[q] = edge_filter_prescreen(r, z0[q], z1[q], z1[q + 1], z0[q + 1]);
        }
        und |= pre[q] & 0xAu;                                // (a 2 in either field)
        inv[q] = (pre[q] & 1u) | ((pre[q] >> 1) & 2u);       // decided: 1 -> removed
    }
    if (und) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (pre[q] & 0xAu) inv[q] = edge_filter_cell(f, i, j0 + q, of_by_one, xr[q], xr[q + 1], y0r, y1r, pre[q], z0[q], z1[q], z1[q + 1], z0[q + 1]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        w1 |= (inv[q] & 1u) << (8 * q);
        w2 |= ((inv[q] >> 1) & 1u) << (8 * q);
        any |= inv[q];
    }
    const size_t ncell = (size_t)(W - 1) * (H - 1);
    const size_t cell = (size_t)i * (W - 1) + j0;
    if (tri_invalid) {
        uint8_t* t = tri_invalid + (size_t)fr * tri_stride;
        if (five) {
            *(u32_unaligned_t*)(t + cell) = w1;
            *(u32_unaligned_t*)(t + ncell + cell) = w2;
        } else {
#pragma unroll
            for (int q = 0; q < 3; ++q) { t[cell + q] = (w1 >> (8 * q)) & 1u; t[ncell + cell + q] = (w2 >> (8 * q)) & 1u; }
        }
    }
    if (unused && any) {
        uint8_t* u = unused + (size_t)fr * unused_stride;
#pragma unroll
        for (int q = 0; q < 4; ++q) if (inv[q]) edge_filter_mark_unused(u, W, i, j0 + q, inv[q]);
    }
}

hipError_t launch_edge_filter(const uint8_t* depth_rgb, size_t pitch, size_t stride, const FrameDev* fp, int frame0,
                              int n, int W, int H, int of_by_one, uint8_t* tri_invalid, size_t tri_stride,
                              uint8_t* unused, size_t unused_stride, hipStream_t s)
{
    const float sx = of_by_one ? (float)(((double)W + 1.0) / (double)W) : 1.0f;
    const float sy = of_by_one ? (float)(((double)H + 1.0) / (double)H) : 1.0f;
    const bool dwords = W % 4 == 0 && W >= 8 && pitch % 4 == 0 && stride % 4 == 0 && ((uintptr_t)depth_rgb % 4) == 0;
    if (dwords) {
        dim3 grid((W / 4 + 127) / 128, H - 1, n);
        hipLaunchKernelGGL(k_edge_filter4, grid, dim3(128), 0, s, depth_rgb, pitch, stride, fp, frame0, W, H, of_by_one,
                           sx, sy, tri_invalid, tri_stride, unused, unused_stride);
    } else {
        dim3 grid((W - 1 + 127) / 128, H - 1, n);
        hipLaunchKernelGGL(k_edge_filter, grid, dim3(128), 0, s, depth_rgb, pitch, stride, fp, frame0, W, H, of_by_one,
                           sx, sy, tri_invalid, tri_stride, unused, unused_stride);
    }
    return hipGetLastError();
}

}  // namespace mdvt
