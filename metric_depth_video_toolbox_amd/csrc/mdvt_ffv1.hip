// mdvt_ffv1.hip -- FFV1 encoding of device frames (mdvt_encode_video_frames): the same packets as the host encoder
// (mdvt_ffv1_encode_frame in csrc_host/mdvt_video.cpp: version 3.4, range coder with the default state table, intra-only, RGB,
// 8 bits, 666 contexts, slices_h x slices_v slices each followed by its 24-bit size, a zero error byte and a CRC-32).
//
// Every slice of every frame of a pass is an independent range coder.  Three launches per pass:
//   k_ffv1_code    one workgroup (one wave) per slice.  The slice's two context-state sets (2 x 666 x 32 B) live in LDS.  In
//                  chunks of kRecChunk samples in coding order (row, then plane, then x) the 64 lanes compute each sample's
//                  (context, sign-adjusted folded difference) record from the pixels -- RCT, median predictor, quant11 context,
//                  with the host's edge rules -- into LDS; lane 0 then range-codes the chunk into the slice's scratch area.
//                  Writes the payload size, or a flag when the payload would pass the slice's capacity (kSliceOverflow) or
//                  the 24-bit slice size (kSliceTooLarge).  Every loop is bounded by the slice's sample count or capacity.
//   k_ffv1_layout  one workgroup: per frame the packet size (payload + 8 per slice) and, in frame order, its offset in the
//                  caller's packet buffer; a frame with a flagged slice, or one that does not fit the buffer, gets a flag size.
//   k_ffv1_emit    one workgroup per slice: copies the payload to its place in the packet, appends the size bytes and the
//                  error byte, and the CRC-32 of both: the lanes take contiguous chunks, each chunk's CRC is shifted over the
//                  bytes behind it (multiplication by x^(8 n) mod P in GF(2)) and the shifted CRCs are XORed.
#include "mdvt_internal.h"
#include "mdvt_ffv1_core.h"

namespace mdvt {
namespace {

constexpr int kFfv1Threads = 64;
using mdvt_ffv1::kStateBytes;                               // one state set: 666 contexts x 32 B (mdvt_ffv1_core.h, with the tables and the CRC algebra)
using mdvt_ffv1::quant11;
using mdvt_ffv1::median3;
using mdvt_ffv1::crc_shift;
constexpr int kRecChunk = 2048;                             // records per coding chunk (8 KiB of LDS)

struct SliceGeom { int x0, y0, sw, sh; };

__device__ __forceinline__ SliceGeom slice_geom(int W, int H, int nh, int nv, int sx, int sy)
{
    SliceGeom g;
    g.x0 = (int)((long long)sx * W / nh);
    g.y0 = (int)((long long)sy * H / nv);
    g.sw = (int)((long long)(sx + 1) * W / nh) - g.x0;
    g.sh = (int)((long long)(sy + 1) * H / nv) - g.y0;
    return g;
}

// the RCT sample of plane p at slice row yy, column xx (rows above the slice read as zero)
__device__ __forceinline__ int rct_sample(const Ffv1CodeArgs& a, const uint8_t* frame, const SliceGeom& g, int p, int yy, int xx)
{
    if (yy < 0) return 0;
    const uint8_t* px = frame + (size_t)(g.y0 + yy) * a.pitch + (size_t)(g.x0 + xx) * (size_t)a.channels;
    int r = px[a.ri], gg = px[a.gi], b = px[a.bi];
    b -= gg; r -= gg;
    gg += (b + r) >> 2;
    return p == 0 ? gg : p == 1 ? b + 256 : r + 256;
}

// record of the sample r of the slice's coding order: (plane != 0) << 19 | context << 9 | (folded difference & 511)
__device__ __forceinline__ uint32_t make_record(const Ffv1CodeArgs& a, const uint8_t* frame, const SliceGeom& g, uint32_t r)
{
    const uint32_t per_row = 3u * (uint32_t)g.sw;
    const int y = (int)(r / per_row);
    const uint32_t rem = r - (uint32_t)y * per_row;
    const int p = (int)(rem / (uint32_t)g.sw);
    const int x = (int)(rem - (uint32_t)p * (uint32_t)g.sw);
    // the host's line buffers: cur[-1] = last[0], last[sw] = last[sw - 1], last[-1] = the row above's cur[-1]
    const int cur = rct_sample(a, frame, g, p, y, x);
    const int T = rct_sample(a, frame, g, p, y - 1, x);
    const int RT = rct_sample(a, frame, g, p, y - 1, x + 1 < g.sw ? x + 1 : g.sw - 1);
    const int L = x > 0 ? rct_sample(a, frame, g, p, y, x - 1) : T;
    const int LT = x > 0 ? rct_sample(a, frame, g, p, y - 1, x - 1) : rct_sample(a, frame, g, p, y - 2, 0);
    int context = quant11((L - LT) & 0xFF) + 11 * quant11((LT - T) & 0xFF) + 121 * quant11((T - RT) & 0xFF);
    int diff = cur - median3(L, T, L + T - LT);
    if (context < 0) { context = -context; diff = -diff; }
    diff = ((diff + 256) & 511) - 256;                     // fold(diff, 9)
    return (p ? 1u << 19 : 0u) | ((uint32_t)context << 9) | ((uint32_t)diff & 511u);
}

// the host's RacEnc, for lane 0: bytes beyond `cap` are counted, not written
struct Rac {
    int low, range, ocount, obyte;
    uint32_t n, cap;
    uint8_t* out;
};

__device__ __forceinline__ void rac_emit(Rac& c, int b)
{
    if (c.n < c.cap) c.out[c.n] = (uint8_t)b;
    ++c.n;
}

__device__ __forceinline__ void rac_renorm(Rac& c)
{
    while (c.range < 0x100) {                              // (at most twice: range >= 1 after any decision)
        if (c.obyte < 0) c.obyte = c.low >> 8;
        else if (c.low <= 0xFF00) {
            rac_emit(c, c.obyte);
            for (; c.ocount; --c.ocount) rac_emit(c, 0xFF);
            c.obyte = c.low >> 8;
        } else if (c.low >= 0x10000) {
            rac_emit(c, c.obyte + 1);
            for (; c.ocount; --c.ocount) rac_emit(c, 0x00);
            c.obyte = (c.low >> 8) & 0xFF;
        } else ++c.ocount;
        c.low = (c.low & 0xFF) << 8;
        c.range <<= 8;
    }
}

__device__ __forceinline__ void rac_put(Rac& c, uint8_t* state, int bit, const uint8_t* zero, const uint8_t* one)
{
    const int s = *state;
    const int range1 = (c.range * s) >> 8;
    if (!bit) { c.range -= range1; *state = zero[s]; }
    else { c.low += c.range - range1; c.range = range1; *state = one[s]; }
    rac_renorm(c);
}

__device__ __forceinline__ void put_symbol(Rac& c, uint8_t* state, int v, bool is_signed, const uint8_t* zero, const uint8_t* one)
{
    if (!v) { rac_put(c, state, 1, zero, one); return; }
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    const int e = 31 - __clz((int)a);
    rac_put(c, state, 0, zero, one);
    for (int i = 0; i < e; ++i) rac_put(c, state + 1 + (i < 9 ? i : 9), 1, zero, one);
    rac_put(c, state + 1 + (e < 9 ? e : 9), 0, zero, one);
    for (int i = e - 1; i >= 0; --i) rac_put(c, state + 22 + (i < 9 ? i : 9), (int)((a >> i) & 1u), zero, one);
    if (is_signed) rac_put(c, state + 11 + (e < 10 ? e : 10), v < 0, zero, one);
}

__global__ void __launch_bounds__(kFfv1Threads) k_ffv1_code(Ffv1CodeArgs a, Ffv1StateTables tab)
{
    __shared__ uint8_t s_st[2 * kStateBytes];
    __shared__ uint32_t s_rec[kRecChunk];
    __shared__ uint8_t s_zero[256], s_one[256];
    __shared__ uint8_t s_misc[64];                         // the slice header's 32 states, the key-frame and terminator states
    __shared__ int s_stop;
    const int tid = (int)threadIdx.x;
    const int spf = a.nh * a.nv;
    const int i = (int)blockIdx.x;                         // slice of the pass
    const int f = i / spf, si = i - f * spf;
    const int sx = si % a.nh, sy = si / a.nh;
    const SliceGeom g = slice_geom(a.W, a.H, a.nh, a.nv, sx, sy);
    const uint8_t* frame = a.src + (size_t)f * a.frame_stride;

    uint32_t* st32 = reinterpret_cast<uint32_t*>(s_st);
    for (int k = tid; k < 2 * kStateBytes / 4; k += kFfv1Threads) st32[k] = 0x80808080u;
    for (int k = tid; k < 256; k += kFfv1Threads) { s_zero[k] = tab.zero[k]; s_one[k] = tab.one[k]; }
    if (tid < 64) s_misc[tid] = 128;
    if (tid == 0) s_stop = 0;
    __syncthreads();

    Rac c;
    c.low = 0; c.range = 0xFF00; c.ocount = 0; c.obyte = -1;
    c.n = 0; c.cap = a.cap; c.out = a.scratch + (size_t)i * a.slice_stride;
    if (tid == 0) {
        if (si == 0) rac_put(c, &s_misc[32], 1, s_zero, s_one);       // every frame is a key frame
        uint8_t* hs = s_misc;
        put_symbol(c, hs, sx, false, s_zero, s_one);
        put_symbol(c, hs, sy, false, s_zero, s_one);
        put_symbol(c, hs, 0, false, s_zero, s_one);          // slice_width - 1, slice_height - 1 (in slice units)
        put_symbol(c, hs, 0, false, s_zero, s_one);
        put_symbol(c, hs, 0, false, s_zero, s_one);          // quant_table_set_index: luma, chroma
        put_symbol(c, hs, 0, false, s_zero, s_one);
        put_symbol(c, hs, 3, false, s_zero, s_one);          // picture_structure: progressive
        put_symbol(c, hs, 0, false, s_zero, s_one);          // sar_num, sar_den
        put_symbol(c, hs, 0, false, s_zero, s_one);
    }
    const uint32_t total = 3u * (uint32_t)g.sw * (uint32_t)g.sh;
    for (uint32_t r0 = 0; r0 < total; r0 += kRecChunk) {
        const uint32_t m = total - r0 < (uint32_t)kRecChunk ? total - r0 : (uint32_t)kRecChunk;
        for (uint32_t k = (uint32_t)tid; k < m; k += kFfv1Threads) s_rec[k] = make_record(a, frame, g, r0 + k);
        __syncthreads();
        if (tid == 0) {
            for (uint32_t k = 0; k < m; ++k) {
                const uint32_t rec = s_rec[k];
                int v = (int)(rec & 511u);
                v = v >= 256 ? v - 512 : v;
                uint8_t* states = s_st + ((rec >> 19) ? kStateBytes : 0) + ((rec >> 9) & 1023u) * 32u;
                put_symbol(c, states, v, true, s_zero, s_one);
            }
            if (c.n > c.cap) s_stop = 1;                   // the payload passes the capacity: no need to go on
        }
        __syncthreads();
        if (s_stop) break;
    }
    if (tid == 0) {
        if (!s_stop) {
            s_misc[33] = 129;                              // terminate(true): the Golomb-Rice sentinel bit, then the flush
            rac_put(c, &s_misc[33], 0, s_zero, s_one);
            c.range = 0xFF; c.low += 0xFF; rac_renorm(c);
            c.range = 0xFF; rac_renorm(c);
        }
        uint32_t res = c.n;
        if (c.n > c.cap) res = a.cap_is_24bit ? kSliceTooLarge : kSliceOverflow;
        a.slice_n[i] = res;
    }
}

__global__ void __launch_bounds__(kFfv1Threads) k_ffv1_layout(Ffv1LayoutArgs a)
{
    const int tid = (int)threadIdx.x;
    for (int f = tid; f < a.n_frames; f += kFfv1Threads) {
        unsigned long long size = 0;
        uint32_t flag = 0;
        for (int k = 0; k < a.spf; ++k) {
            const uint32_t v = a.slice_n[(size_t)f * a.spf + k];
            if (v >= kSliceTooLarge) { if (flag != kSliceTooLarge) flag = v; }
            else size += (unsigned long long)v + 8u;
        }
        if (!flag && size >= kSliceTooLarge) flag = kSliceOverflow;
        a.sizes[f] = flag ? flag : (uint32_t)size;
    }
    __syncthreads();
    if (tid == 0) {                                        // frame order: the offsets of this pass follow the earlier passes'
        unsigned long long base = *a.used;
        for (int f = 0; f < a.n_frames; ++f) {
            uint32_t sz = a.sizes[f];
            if (sz < kSliceTooLarge && base + sz > a.packets_cap) { sz = kSliceOverflow; a.sizes[f] = sz; }
            a.offsets[f] = base;
            if (sz < kSliceTooLarge) base += sz;
        }
        *a.used = base;
    }
}

__global__ void __launch_bounds__(kFfv1Threads) k_ffv1_emit(Ffv1EmitArgs a)
{
    __shared__ uint32_t s_crc[256];
    __shared__ uint32_t s_part[kFfv1Threads];
    const int tid = (int)threadIdx.x;
    const int i = (int)blockIdx.x;
    const int f = i / a.spf, si = i - f * a.spf;
    const uint32_t fsize = a.sizes[f];
    if (fsize >= kSliceTooLarge) return;                   // flagged frame: nothing is written
    for (int k = tid; k < 256; k += kFfv1Threads) {
        s_crc[k] = mdvt_ffv1::crc_table_entry((uint32_t)k);
    }
    // this slice's place: the frame's offset + the earlier slices of the frame
    unsigned long long before = 0;
    for (int k = tid; k < si; k += kFfv1Threads) before += (unsigned long long)a.slice_n[(size_t)f * a.spf + k] + 8u;
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
    const uint32_t n = a.slice_n[i];
    const uint8_t* src = a.scratch + (size_t)i * a.slice_stride;
    uint8_t* dst = a.packets + a.offsets[f] + before;
    __syncthreads();
    const uint32_t per = (n + kFfv1Threads - 1) / kFfv1Threads;
    const uint32_t b0 = per * (uint32_t)tid < n ? per * (uint32_t)tid : n;
    const uint32_t b1 = b0 + per < n ? b0 + per : n;
    uint32_t crc = 0;
    for (uint32_t k = b0; k < b1; ++k) {
        const uint8_t v = src[k];
        dst[k] = v;
        crc = (crc << 8) ^ s_crc[(crc >> 24) ^ v];
    }
    s_part[tid] = crc_shift(crc, n - b1);
    __syncthreads();
    if (tid == 0) {
        uint32_t all = 0;
        for (int k = 0; k < kFfv1Threads; ++k) all ^= s_part[k];
        const uint8_t tail[4] = {(uint8_t)(n >> 16), (uint8_t)(n >> 8), (uint8_t)n, 0};     // 24-bit size, error_status
        for (int k = 0; k < 4; ++k) {
            dst[n + k] = tail[k];
            all = (all << 8) ^ s_crc[(all >> 24) ^ tail[k]];
        }
        dst[n + 4] = (uint8_t)(all >> 24); dst[n + 5] = (uint8_t)(all >> 16); dst[n + 6] = (uint8_t)(all >> 8); dst[n + 7] = (uint8_t)all;
    }
}

}  // namespace

// the default state-transition table (RFC 9043 section 3.8.1.3), built as the host encoder builds it
Ffv1StateTables ffv1_default_states()
{
    Ffv1StateTables s;
    mdvt_ffv1::default_states(s.zero, s.one);
    return s;
}

hipError_t launch_ffv1_code(const Ffv1CodeArgs& a, const Ffv1StateTables& tab, int n_slices, hipStream_t s)
{
    hipLaunchKernelGGL(k_ffv1_code, dim3(n_slices), dim3(kFfv1Threads), 0, s, a, tab);
    return hipGetLastError();
}

hipError_t launch_ffv1_layout(const Ffv1LayoutArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_ffv1_layout, dim3(1), dim3(kFfv1Threads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ffv1_emit(const Ffv1EmitArgs& a, int n_slices, hipStream_t s)
{
    hipLaunchKernelGGL(k_ffv1_emit, dim3(n_slices), dim3(kFfv1Threads), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdvt
