// mdvt_scene.hip -- the difference sums behind scene detection (mdvt_scene_frame_sums, include/mdvt_scene.h): per pair of consecutive
// frames the exact integers sum |dH|, sum |dS|, sum |dV| over the analysed image, H, S, V being OpenCV's 8-bit COLOR_BGR2HSV as the
// header restates it.
//
// Layout.  A thread owns a fixed set of pixels of the analysed image, walks the frames of the call and keeps the previous frame's
// H, S, V of its pixels in registers (one packed dword per pixel): a frame's bytes are read from memory once, and no workspace is
// needed.  Per pair the thread's three sums are reduced over the wave by shuffles, over the workgroup's four waves through LDS (two
// buffers taken in turn, so one barrier per frame), and three threads add the workgroup's sums to the caller's 64-bit words with
// integer atomics: the result is exact and independent of the order.  A workgroup's sums fit 32 bits (256 threads x 16 pixels x 255).
//   k_scene_vec    factor 1, every base, pitch and stride a multiple of 16: a thread owns 16 consecutive pixels of a row, 48 bytes
//                  in three 16-byte loads; the next frame's loads are issued before the current frame's arithmetic.  The last group of
//                  a row whose length is no multiple of 16 is read byte by byte.
//   k_scene_px     everything else: a thread owns one pixel of the analysed image, mdvt_adapter_resize.h's u8 resize over byte loads
//                  (mode 0, the copy, is the byte path of factor 1; mode 1 the exact 2 x area mean; mode 2 the linear taps).
// The two division tables (256 words each) are built per workgroup in LDS with integer arithmetic: rint(N / double(i)) is the
// quotient rounded to nearest, ties to even, and N / i is never within 2^-52 of a tie it does not hit (i <= 1530).
#include "mdvt_internal.h"
#include "mdvt_adapter_resize.h"

namespace mdvt {
namespace {

constexpr int kThreads = 256;
constexpr int kGroup = 16;            // pixels a thread of k_scene_vec owns

struct Tables { int sdiv[256], hdiv[256]; };

__device__ __forceinline__ int div_rne(int n, int i)
{
    const int q = n / i, r = n - q * i;
    return 2 * r > i ? q + 1 : (2 * r == i ? q + (q & 1) : q);
}

__device__ __forceinline__ void build_tables(Tables& t)
{
    const int i = (int)threadIdx.x;              // kThreads == 256
    t.sdiv[i] = i ? div_rne(255 << 12, i) : 0;
    t.hdiv[i] = i ? div_rne((180 << 12) / 6, i) : 0;          // (180 << 12) / (6 i); 180 << 12 is a multiple of 6
}

// H | S << 8 | V << 16 of a pixel given as byte 0 | byte 1 << 8 | byte 2 << 16
__device__ __forceinline__ uint32_t hsv_of(const Tables& t, uint32_t px, int bgr)
{
    const int b0 = (int)(px & 0xFFu), g = (int)((px >> 8) & 0xFFu), b2 = (int)((px >> 16) & 0xFFu);
    const int r = bgr ? b2 : b0, b = bgr ? b0 : b2;
    const int v = max(r, max(g, b)), m = min(r, min(g, b)), d = v - m;
    const int S = min(255, (d * t.sdiv[v] + 2048) >> 12);
    const int h = v == r ? g - b : (v == g ? b - r + 2 * d : r - g + 4 * d);
    int H = (h * t.hdiv[d] + 2048) >> 12;
    if (H < 0) H += 180;
    return (uint32_t)H | ((uint32_t)S << 8) | ((uint32_t)v << 16);
}

__device__ __forceinline__ int absdiff8(uint32_t a, uint32_t b, int shift)
{
    const int d = (int)((a >> shift) & 0xFFu) - (int)((b >> shift) & 0xFFu);
    return d < 0 ? -d : d;
}

struct Sums3 { uint32_t h, s, v; };

__device__ __forceinline__ void add_diff(Sums3& acc, uint32_t a, uint32_t b)
{
    acc.h += (uint32_t)absdiff8(a, b, 0);
    acc.s += (uint32_t)absdiff8(a, b, 8);
    acc.v += (uint32_t)absdiff8(a, b, 16);
}

// The workgroup's sums of one pair to the caller's three words.  `part` is the buffer of this pair (two are taken in turn).
__device__ __forceinline__ void reduce_pair(Sums3 acc, uint32_t (*part)[3], unsigned long long* out)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        acc.h += __shfl_xor(acc.h, m);
        acc.s += __shfl_xor(acc.s, m);
        acc.v += __shfl_xor(acc.v, m);
    }
    const int tid = (int)threadIdx.x;
    if ((tid & 63) == 0) {
        part[tid >> 6][0] = acc.h;
        part[tid >> 6][1] = acc.s;
        part[tid >> 6][2] = acc.v;
    }
    __syncthreads();
    if (tid < 3) {
        const uint32_t v = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
        if (v) atomicAdd(out + tid, (unsigned long long)v);
    }
}

// ---- factor 1, 16-byte loads ---------------------------------------------------------------------------------------------------
struct Raw { uint32_t w[12]; };       // 16 pixels: 48 bytes

__device__ __forceinline__ Raw load_raw(const uint8_t* p, int cnt)
{
    Raw r;
    if (cnt == kGroup) {
        const uint4* q = reinterpret_cast<const uint4*>(p);
        const uint4 a = q[0], b = q[1], c = q[2];
        r.w[0] = a.x; r.w[1] = a.y; r.w[2] = a.z; r.w[3] = a.w;
        r.w[4] = b.x; r.w[5] = b.y; r.w[6] = b.z; r.w[7] = b.w;
        r.w[8] = c.x; r.w[9] = c.y; r.w[10] = c.z; r.w[11] = c.w;
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            uint32_t w = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * k + j < 3 * cnt) w |= (uint32_t)p[4 * k + j] << (8 * j);        // (bytes of the row's own pixels only)
            r.w[k] = w;
        }
    }
    return r;
}

__device__ __forceinline__ uint32_t raw_px(const Raw& r, int k)
{
    // pixel k is bytes 3 k .. 3 k + 2 (k is a constant after unrolling)
    const int at = 3 * k, w = at >> 2, sh = 8 * (at & 3);
    uint32_t v = r.w[w] >> sh;
    if (sh > 8) v |= r.w[w + 1] << (32 - sh);
    return v & 0xFFFFFFu;
}

__global__ void __launch_bounds__(kThreads) k_scene_vec(SceneArgs a)
{
    __shared__ Tables tab;
    __shared__ uint32_t part[2][4][3];
    build_tables(tab);
    __syncthreads();
    const uint32_t gid = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    const bool active = gid < a.units;
    uint32_t row = 0, gx = 0;
    if (active) { row = gid / a.gw; gx = gid - row * a.gw; }
    const int cnt = active ? (int)min((uint32_t)kGroup, a.W - gx * (uint32_t)kGroup) : 0;
    const size_t col = (size_t)gx * (size_t)(3 * kGroup);
    const uint8_t* at = a.frames + (size_t)row * a.pitch + col;

    uint32_t last[kGroup];
    int f = 0;
    {
        const Raw r0 = active ? load_raw(a.prev ? a.prev + (size_t)row * a.prev_pitch + col : at, cnt) : Raw{};
        if (!a.prev) f = 1;
#pragma unroll
        for (int k = 0; k < kGroup; ++k) last[k] = hsv_of(tab, raw_px(r0, k), a.bgr);
    }
    unsigned long long* out = a.sums;
    Raw cur = (active && f < a.n_frames) ? load_raw(at + (size_t)f * a.stride, cnt) : Raw{};
    for (int i = 0; f < a.n_frames; ++f, ++i, out += 3) {
        Raw nxt{};
        if (active && f + 1 < a.n_frames) nxt = load_raw(at + (size_t)(f + 1) * a.stride, cnt);
        Sums3 acc{0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < kGroup; ++k) {
            const uint32_t c = hsv_of(tab, raw_px(cur, k), a.bgr);
            if (k < cnt) add_diff(acc, c, last[k]);
            last[k] = c;
        }
        reduce_pair(acc, part[i & 1], out);
        cur = nxt;
    }
}

// ---- one analysed pixel per thread, byte loads ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_scene_px(SceneArgs a)
{
    __shared__ Tables tab;
    __shared__ uint32_t part[2][4][3];
    build_tables(tab);
    __syncthreads();
    const uint32_t gid = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    const bool active = gid < a.units;
    int x = 0, y = 0;
    if (active) { y = (int)(gid / (uint32_t)a.rs.out_w); x = (int)(gid - (uint32_t)y * (uint32_t)a.rs.out_w); }
    auto hsv_at = [&](const uint8_t* frame, size_t pitch) {
        const uint32_t px = adapter_resize_px(a.rs, x, y, [&](int sx, int sy) { return load_px_bytes(frame + (size_t)sy * pitch, sx); });
        return hsv_of(tab, px, a.bgr);
    };
    int f = a.prev ? 0 : 1;
    uint32_t last = 0;
    if (active) last = a.prev ? hsv_at(a.prev, a.prev_pitch) : hsv_at(a.frames, a.pitch);
    unsigned long long* out = a.sums;
    for (int i = 0; f < a.n_frames; ++f, ++i, out += 3) {
        Sums3 acc{0u, 0u, 0u};
        if (active) {
            const uint32_t c = hsv_at(a.frames + (size_t)f * a.stride, a.pitch);
            add_diff(acc, c, last);
            last = c;
        }
        reduce_pair(acc, part[i & 1], out);
    }
}

}  // namespace

hipError_t launch_scene_sums(const SceneArgs& a, bool vec, hipStream_t s)
{
    const dim3 grid((a.units + (uint32_t)kThreads - 1u) / (uint32_t)kThreads);
    if (vec) hipLaunchKernelGGL(k_scene_vec, grid, dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL(k_scene_px, grid, dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdvt
