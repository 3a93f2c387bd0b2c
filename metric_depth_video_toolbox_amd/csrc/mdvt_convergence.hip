// mdvt_convergence.hip -- per-frame masked depth means (mdvt_convergence_depths, include/mdvt_convergence.h): the number the
// reference's find_convergence_depth.py:53-80 takes per frame, `depth[gray > 240].mean()` in float32, bit for bit.
//
// The value.  code = R << 24 | B << 16 of the depth pixel; depth = float(code) / float(255^4 / max_depth), ONE correctly rounded
// float32 division (fcd:60) -- not the render's decode, which multiplies by max_depth / 255^4 (dfh:21-23) and rounds differently.
// The unit is compiled with -fhip-fp32-correctly-rounded-divide-sqrt and without fast-math (Makefile): `/` below is IEEE.
//
// The order.  NumPy's float32 mean of n contiguous values: consecutive chunks of 8192 (the ufunc buffer), each summed by the pairwise
// routine pw(a, n) -- n < 8: in order; n <= 128: eight strided accumulators, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the last n % 8
// in order; else pw(a, n2) + pw(a + n2, n - n2) with n2 = n / 2 rounded down to a multiple of 8 -- the chunk sums added one after the
// other, the total divided by float(n).  A full chunk is a balanced tree over 64 leaves of 128 values; a tail chunk has at most 128
// leaves at depths of at most 7.  Every sum below has a fixed shape: no floating-point atomics, no dependence on launch geometry.
//
// Launches per launch set (frames that have a mask frame take all five, the others the last two):
//   k_conv_select   one wave per unit of 2048 pixels of the mask: gray = (4899 R + 9617 G + 1868 B + 8192) >> 14 > 240 (OpenCV's 8-bit
//                   BGR2GRAY), the selection as ballot words (lane l holds pixels 4 l .. 4 l + 3 of a group of 256) and the unit's count
//   k_conv_scan     one wave per frame: exclusive scan of the unit counts, the frame's count (mdvt_ordered_select.h: unit_scan)
//   k_conv_compact  one wave per unit: the 16-bit codes R << 8 | B of the selected pixels, in row-major order, to their places; depth
//                   pixels are loaded only by lanes that hold a selected one
//   k_conv_reduce   one workgroup of four waves per chunk of 8192 values: the codes are staged in LDS (coalesced 12-byte loads of four
//                   pixels when the row length, pitch, stride and base are multiples of 4, else bytes), four padding dwords per leaf,
//                   so that the four threads of a leaf -- two of its eight accumulators each -- read without bank conflicts; a full
//                   chunk is 64 leaf sums and a balanced tree of butterfly steps over the lanes, then over the waves (IEEE add is
//                   commutative: both sides hold the same bits); a tail chunk is walked in the general shape (leaves listed by
//                   thread 0, summed by a thread each, combined by thread 0)
//   k_conv_mean     one wave per frame: the chunk sums in order, the division, the NaN of an empty selection (mdvt_ordered_select.h:
//                   ordered_mean), the count
// The scan and the mean are shared with the focal estimate of mdvt_depth_engines.hip; select, compact and reduce are this unit's own.
#include "mdvt_internal.h"
#include "mdvt_ordered_select.h"

namespace mdvt {
namespace {

using pairwise::kChunk;               // NumPy's ufunc buffer, in elements
using pairwise::kLeaf;                // the pairwise routine's block
constexpr int kUnit = 2048;           // pixels a wave selects / compacts
constexpr int kGroup = 256;           // pixels of one step of a wave: four per lane

struct Px4 { uint32_t v[4]; };        // four pixels, byte 0 | byte 1 << 8 | byte 2 << 16 each

// pixels p .. p + 3 in row-major order of a frame of npx pixels, rows of W (npx where the rows have no padding: no division then);
// pixels from npx on read as 0 and touch no memory.
// vec: p, W, the pitch and the frame's address are multiples of 4 -- the four pixels are 12 aligned bytes of one row
__device__ __forceinline__ Px4 load_px4(const uint8_t* frame, size_t pitch, uint32_t W, uint32_t npx, uint32_t p, bool vec)
{
    Px4 o{{0u, 0u, 0u, 0u}};
    if (p >= npx) return o;
    uint32_t row = 0, col = p;
    if (W != npx) { row = p / W; col = p - row * W; }                // (W == npx: rows without padding are one long row)
    if (vec) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(frame + (size_t)row * pitch + (size_t)col * 3u);
        const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
        o.v[0] = w0 & 0xFFFFFFu;
        o.v[1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
        o.v[2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
        o.v[3] = w2 >> 8;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (p + (uint32_t)k < npx) {
                const uint8_t* q = frame + (size_t)row * pitch + (size_t)col * 3u;
                o.v[k] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
                if (++col == W) { col = 0; ++row; }
            }
        }
    }
    return o;
}

// R << 8 | B of a depth pixel (G is ignored, fcd:58-59)
__device__ __forceinline__ uint32_t code_of(uint32_t px, int bgr)
{
    const uint32_t lo = px & 0xFFu, hi = (px >> 16) & 0xFFu;
    return (lo << (bgr ? 0 : 8)) | (hi << (bgr ? 8 : 0));          // (uniform shifts)
}

__device__ __forceinline__ bool selected(uint32_t px, int bgr)
{
    const uint32_t lo = px & 0xFFu, g = (px >> 8) & 0xFFu, hi = (px >> 16) & 0xFFu;
    const uint32_t wlo = bgr ? 1868u : 4899u, whi = bgr ? 4899u : 1868u;     // (uniform: the weight of R is 4899, of B 1868)
    return ((wlo * lo + 9617u * g + whi * hi + 8192u) >> 14) > 240u;
}

__device__ __forceinline__ int popc64(unsigned long long v) { return __popcll(v); }

__global__ void __launch_bounds__(256) k_conv_select(ConvergenceArgs a)
{
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t u = blockIdx.x * 4u + (threadIdx.x >> 6);
    const int f = (int)blockIdx.y;
    if (u >= a.nunits) return;
    const uint8_t* frame = a.mask + (size_t)f * a.mask_stride;
    unsigned long long* bits = a.bits + ((size_t)f * a.nunits + u) * (size_t)(kUnit / 64);
    uint32_t cnt = 0;
    for (int g = 0; g < kUnit / kGroup; ++g) {
        const uint32_t p = u * (uint32_t)kUnit + (uint32_t)(g * kGroup + 4 * lane);
        const Px4 q = load_px4(frame, a.mask_pitch, a.mask_W, a.npx, p, a.mask_vec != 0);
        unsigned long long b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            b[k] = __ballot(p + (uint32_t)k < a.npx && selected(q.v[k], a.mask_bgr));
            cnt += (uint32_t)popc64(b[k]);
        }
        if (lane < 4) bits[g * 4 + lane] = lane == 0 ? b[0] : lane == 1 ? b[1] : lane == 2 ? b[2] : b[3];
    }
    if (lane == 0) a.unit_cnt[(size_t)f * a.nunits + u] = cnt;
}

__global__ void __launch_bounds__(64) k_conv_scan(ConvergenceArgs a)
{
    const size_t f = blockIdx.x;
    ordered_select::unit_scan(a.unit_cnt + f * a.nunits, a.unit_off + f * a.nunits, a.nunits, a.totals + f);
}

__global__ void __launch_bounds__(256) k_conv_compact(ConvergenceArgs a)
{
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t u = blockIdx.x * 4u + (threadIdx.x >> 6);
    const int f = (int)blockIdx.y;
    if (u >= a.nunits) return;
    const uint8_t* frame = a.depth + (size_t)f * a.depth_stride;
    const unsigned long long* bits = a.bits + ((size_t)f * a.nunits + u) * (size_t)(kUnit / 64);
    uint16_t* dst = a.compact + (size_t)f * a.compact_stride;
    uint32_t off = a.unit_off[(size_t)f * a.nunits + u];         // < npx, and off + the unit's count <= npx
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int g = 0; g < kUnit / kGroup; ++g) {
        const unsigned long long b0 = bits[g * 4], b1 = bits[g * 4 + 1], b2 = bits[g * 4 + 2], b3 = bits[g * 4 + 3];
        if ((b0 | b1 | b2 | b3) == 0ull) continue;
        if (((b0 | b1 | b2 | b3) >> lane) & 1ull) {
            const uint32_t p = u * (uint32_t)kUnit + (uint32_t)(g * kGroup + 4 * lane);
            const Px4 q = load_px4(frame, a.depth_pitch, a.depth_W, a.npx, p, a.depth_vec != 0);
            uint32_t pos = off + (uint32_t)(popc64(b0 & below) + popc64(b1 & below) + popc64(b2 & below) + popc64(b3 & below));
            if ((b0 >> lane) & 1ull) dst[pos++] = (uint16_t)code_of(q.v[0], a.depth_bgr);
            if ((b1 >> lane) & 1ull) dst[pos++] = (uint16_t)code_of(q.v[1], a.depth_bgr);
            if ((b2 >> lane) & 1ull) dst[pos++] = (uint16_t)code_of(q.v[2], a.depth_bgr);
            if ((b3 >> lane) & 1ull) dst[pos++] = (uint16_t)code_of(q.v[3], a.depth_bgr);
        }
        off += (uint32_t)(popc64(b0) + popc64(b1) + popc64(b2) + popc64(b3));
    }
}

constexpr int kReduceThreads = 256;   // threads that sum one chunk: four per leaf of a full chunk
constexpr int kLeafPad = 4;           // dwords of padding behind every leaf of 128 staged codes: the four threads of eight leaves read 32 banks

// the staged chunk: code i is half (i & 1) of dword (i >> 1) + 4 (i >> 7)
__device__ __forceinline__ int code_dword(int i) { return (i >> 1) + kLeafPad * (i >> 7); }

struct Staged {
    const uint32_t* s;
    float div;
    __device__ __forceinline__ float operator()(int i) const
    {
        const uint32_t d = s[code_dword(i)];
        return (float)(((i & 1) ? d >> 16 : d & 0xFFFFu) << 16) / div;
    }
};

__global__ void __launch_bounds__(kReduceThreads) k_conv_reduce(ConvergenceArgs a)
{
    __shared__ uint32_t s_code[kChunk / 2 + kLeafPad * (kChunk / kLeaf)];
    __shared__ pairwise::Shape s_shape;
    __shared__ float s_val[4];
    const int tid = (int)threadIdx.x;
    const uint32_t c = blockIdx.x;
    const int f = (int)blockIdx.y;
    const bool masked = f < a.n_masked;
    const uint32_t total = masked ? a.totals[f] : a.npx;
    const uint32_t first = c * (uint32_t)kChunk;
    if (first >= total) return;
    const int n = (int)(total - first < (uint32_t)kChunk ? total - first : (uint32_t)kChunk);

    if (masked) {
        const uint16_t* src = a.compact + (size_t)f * a.compact_stride + first;      // 8-byte aligned; the row of codes is padded to 8
#pragma unroll
        for (int g = 0; g < kChunk / (4 * kReduceThreads); ++g) {
            const int i = 4 * (g * kReduceThreads + tid);
            if (i < n) {
                const uint2 w = *reinterpret_cast<const uint2*>(src + i);
                s_code[code_dword(i)] = w.x;
                s_code[code_dword(i) + 1] = w.y;
            }
        }
    } else {
        const uint8_t* frame = a.depth + (size_t)f * a.depth_stride;
#pragma unroll
        for (int g = 0; g < kChunk / (4 * kReduceThreads); ++g) {
            const int i = 4 * (g * kReduceThreads + tid);
            if (i < n) {
                const Px4 q = load_px4(frame, a.depth_pitch, a.depth_W, a.npx, first + (uint32_t)i, a.depth_vec != 0);
                s_code[code_dword(i)] = code_of(q.v[0], a.depth_bgr) | (code_of(q.v[1], a.depth_bgr) << 16);
                s_code[code_dword(i) + 1] = code_of(q.v[2], a.depth_bgr) | (code_of(q.v[3], a.depth_bgr) << 16);
            }
        }
    }
    __syncthreads();

    const Staged v{s_code, a.div};
    if (n == kChunk) {
        // four threads per leaf: thread q of a leaf keeps the accumulators r[2 q] and r[2 q + 1] (a dword of codes per step of 8), the
        // four join as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); then the balanced tree over the wave's 16 leaves, then over
        // the four waves.  IEEE add is commutative: both sides of a butterfly step hold the same bits.
        const uint32_t* leaf = s_code + (tid >> 2) * (kLeaf / 2 + kLeafPad) + (tid & 3);
        uint32_t d = leaf[0];
        float r0 = (float)((d & 0xFFFFu) << 16) / a.div, r1 = (float)((d >> 16) << 16) / a.div;
#pragma unroll
        for (int i = 1; i < kLeaf / 8; ++i) {
            d = leaf[4 * i];
            r0 += (float)((d & 0xFFFFu) << 16) / a.div;
            r1 += (float)((d >> 16) << 16) / a.div;
        }
        float res = r0 + r1;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) res += __shfl_xor(res, m);
        if ((tid & 63) == 0) s_val[tid >> 6] = res;
        __syncthreads();
        if (tid == 0) a.sums[(size_t)f * a.nchunks + c] = (s_val[0] + s_val[1]) + (s_val[2] + s_val[3]);
        return;
    }
    // the general shape (mdvt_pairwise.h): thread 0 lists the leaves, a thread each sums them, thread 0 joins them
    if (tid == 0) pairwise::shape_list(s_shape, n);
    __syncthreads();
    pairwise::shape_leaves(s_shape, v, tid);
    __syncthreads();
    if (tid == 0) a.sums[(size_t)f * a.nchunks + c] = pairwise::shape_join(s_shape);
}

__global__ void __launch_bounds__(64) k_conv_mean(ConvergenceArgs a)
{
    const int f = (int)blockIdx.x;
    const uint32_t total = f < a.n_masked ? a.totals[f] : a.npx;
    const float mean = ordered_select::ordered_mean(a.sums + (size_t)f * a.nchunks, total, __builtin_nanf(""));
    if (threadIdx.x == 0) {
        a.means[f] = mean;
        if (a.counts) a.counts[f] = total;
    }
}

}  // namespace

hipError_t launch_convergence(const ConvergenceArgs& a, hipStream_t s)
{
    if (a.n_masked > 0) {
        const dim3 units((a.nunits + 3u) / 4u, (unsigned)a.n_masked);
        hipLaunchKernelGGL(k_conv_select, units, dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_conv_scan, dim3((unsigned)a.n_masked), dim3(64), 0, s, a);
        hipLaunchKernelGGL(k_conv_compact, units, dim3(256), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_conv_reduce, dim3(a.nchunks, (unsigned)a.n_frames), dim3(kReduceThreads), 0, s, a);
    hipLaunchKernelGGL(k_conv_mean, dim3((unsigned)a.n_frames), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdvt
