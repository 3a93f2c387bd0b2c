// mdvt_ffv1_stream_decode.hip -- FFV1 streams whose context state carries from frame to frame (mdvt_decode_video_stream,
// include/mdvt_ffv1_stream_decode.h): version 3, coder_type 0 (Golomb-Rice with run mode) or 1 (range coder), intra 0 or 1.  The
// bytes mdvt_video_read writes when it reads the same packets in order from a run's key frame.
//
// Where a frame of the intra class is nh x nv independent decoders (mdvt_ffv1_decode.hip), here a slice's decoder of frame k needs
// the state its decoder of frame k - 1 left behind, back to the last key frame.  So the unit of work is (key-frame run, slice): far
// fewer workgroups, each of them serial.  That is the format.  The key frames' positions are only known on the device:
//   k_ffv1_stream_walk    one thread per frame: the packet against the packet buffer, its slice table (walk_slices), and its
//                         key-frame bit from the first two bytes as the range decoder decides it.  Writes the frame's status word
//                         (0 or kBadPacket) and its kind (inter, key, refused).
//   k_ffv1_stream_chain   one workgroup of two waves per (frame, slice).  It leaves at once unless its frame is a key frame;
//                         otherwise it decodes its slice of that frame and of every frame after it up to the next key frame or the
//                         call's end.  The context state lives in LDS through the whole run -- VlcState[2][666] (8 KiB) or two range
//                         state sets (42 KiB) --, reset by the workgroup at the run's start.  Per frame: the slice's CRC (ec), then
//                         lane 0 reads the slice header, claims the slice's cell and decodes row y while the second wave undoes the
//                         RCT of row y - 1 and stores it (not for frames before first_out); one barrier per row, as k_ffv1_dec_slice.
//                         A frame it has to flag ends the chain: every later frame of the run gets kBrokenRun.
//                         The workgroup of (frame 0, slice 0) also flags the frames in front of the call's first key frame.
// Every loop here is bounded by the frame's geometry, the packet's byte count or the number of frames, never by a decoded value.
#include "mdvt_internal.h"
#include "mdvt_ffv1_core.h"

namespace mdvt {
namespace {

using namespace mdvt_ffv1;

constexpr int kChainThreads = 128;
constexpr int kWalkThreads = 64;

struct PacketByte {
    const uint8_t* p;
    __device__ uint8_t operator()(uint32_t k) const { return p[k]; }
};

// the slice's bytes for lane 0: whole aligned 8-byte words where they lie inside [p, p + avail), single bytes at the rims
struct GlobalSrc {
    const uint8_t* p;
    uint32_t avail, wbase;
    unsigned long long w;
    __device__ uint8_t byte(uint32_t k)
    {
        if (k - wbase >= 8u) {
            const unsigned long long addr = (unsigned long long)(p + k) & ~7ull;
            if (addr < (unsigned long long)p || addr + 8u > (unsigned long long)p + avail) return p[k];
            w = *reinterpret_cast<const unsigned long long*>(addr);
            wbase = (uint32_t)(addr - (unsigned long long)p);
        }
        return (uint8_t)(w >> (8u * (k - wbase)));
    }
};

__global__ void __launch_bounds__(kWalkThreads) k_ffv1_stream_walk(Ffv1StreamArgs a)
{
    const int f = (int)(blockIdx.x * kWalkThreads + threadIdx.x);
    if (f >= a.n_frames) return;
    const int spf = a.nh * a.nv;
    const unsigned long long off = a.offsets[f];
    const uint32_t size = a.sizes[f];
    uint32_t st = kBadPacket, kind = kFrameBad;
    if (off <= a.packets_bytes && size <= a.packets_bytes - off) {
        const size_t slices = (size_t)a.n_frames * (size_t)spf;
        const uint8_t* pkt = a.packets + off;
        st = walk_slices(PacketByte{pkt}, size, spf, a.ec, a.table + (size_t)f * spf, a.table + slices + (size_t)f * spf);
        if (st == kOk) kind = key_frame_bit(pkt[0], pkt[1]) ? kFrameKey : kFrameInter;      // (size >= 3: walk_slices)
    }
    a.status[f] = st;
    a.kind[f] = kind;
}

__global__ void __launch_bounds__(kChainThreads) k_ffv1_stream_chain(Ffv1StreamArgs a, Ffv1StateTables tab)
{
    __shared__ uint16_t s_next[256];                       // zero_state | one_state << 8
    __shared__ uint8_t s_misc[64];
    __shared__ int8_t s_q11[256];
    __shared__ uint32_t s_part[kChainThreads];
    __shared__ int s_geom[5];                              // status, x0, y0, sw, sh
    extern __shared__ uint32_t s_dyn[];                    // the context state, then 3 planes x 3 slots x line_stride samples
    const int tid = (int)threadIdx.x;
    const int spf = a.nh * a.nv;
    const int f0 = (int)blockIdx.x / spf, si = (int)blockIdx.x - f0 * spf;
    if (a.kind[f0] != kFrameKey) {
        // the frames in front of the call's first key frame belong to no chain
        if (f0 == 0 && si == 0 && tid == 0)
            for (int j = 0; j < a.n_frames && a.kind[j] != kFrameKey; ++j) atomicMax(&a.status[j], kNoKeyFrame);
        return;
    }
    const uint32_t state_bytes = 2u * (uint32_t)(a.coder ? kStateBytes : kVlcBytes);     // (both multiples of 4)
    uint8_t* s_st = reinterpret_cast<uint8_t*>(s_dyn);
    int16_t* s_lines = reinterpret_cast<int16_t*>(s_st + state_bytes);
    uint32_t* s_crc = reinterpret_cast<uint32_t*>(s_lines);                              // (the CRC table borrows the rows' place)
    const size_t slices = (size_t)a.n_frames * (size_t)spf;
    const uint32_t trailer = a.ec ? 8u : 3u;

    for (int k = tid; k < 256; k += kChainThreads) { s_next[k] = (uint16_t)(tab.zero[k] | (tab.one[k] << 8)); s_q11[k] = (int8_t)quant11(k); }
    if (a.coder) {
        for (uint32_t k = tid; k < state_bytes / 4u; k += kChainThreads) s_dyn[k] = 0x80808080u;
    } else {
        VlcState* vs = reinterpret_cast<VlcState*>(s_st);
        for (int k = tid; k < 2 * kContexts; k += kChainThreads) vlc_reset(vs + k);
    }

    ChainDec<GlobalSrc> d;
    d.st = s_st; d.lines = s_lines; d.misc = s_misc; d.q11 = s_q11; d.stride = a.line_stride;
    int f = f0;
    uint32_t flag = kOk;                                   // why the chain ends at frame f (uniform across the workgroup)
    for (; f < a.n_frames; ++f) {
        const uint32_t kind = a.kind[f];                   // (written by the walk alone: the same word for every thread)
        if (f > f0 && kind == kFrameKey) break;            // the next run's workgroup takes over
        if (kind == kFrameBad) { flag = kBadPacket; break; }
        const size_t i = (size_t)f * spf + (size_t)si;
        const uint32_t off = a.table[i], len = a.table[slices + i];
        const uint8_t* data = a.packets + a.offsets[f] + off;      // [data, data + len + trailer) lies inside the packet (the walk)
        __syncthreads();                                   // the last frame's rows are stored; the tables and the state are set
        if (a.ec) {
            for (int k = tid; k < 256; k += kChainThreads) s_crc[k] = crc_table_entry((uint32_t)k);
            __syncthreads();
            const uint32_t n = len + trailer;
            const uint32_t per = (n + kChainThreads - 1) / kChainThreads;
            const uint32_t b0 = per * (uint32_t)tid < n ? per * (uint32_t)tid : n;
            const uint32_t b1 = b0 + per < n ? b0 + per : n;
            uint32_t crc = 0;
            for (uint32_t k = b0; k < b1; ++k) crc = (crc << 8) ^ s_crc[(crc >> 24) ^ data[k]];
            s_part[tid] = crc_shift(crc, n - b1);
            __syncthreads();
            if (tid == 0) {
                uint32_t all = 0;
                for (int k = 0; k < kChainThreads; ++k) all ^= s_part[k];
                s_geom[0] = all ? (int)kCrcMismatch : 0;
            }
            __syncthreads();
            if (s_geom[0] != 0) { flag = kCrcMismatch; break; }
        }
        for (int k = tid; k < 9 * a.line_stride; k += kChainThreads) s_lines[k] = 0;
        __syncthreads();
        if (tid == 0) {
            GlobalSrc src;
            src.p = data; src.avail = len + trailer; src.wbase = 0xFFFFFF00u; src.w = 0;
            uint32_t st = d.begin(src, len + trailer, len, si == 0, a.coder, a.micro, a.W, a.H, a.nh, a.nv, s_next);
            if (st == kOk && atomicExch(&a.claims[(size_t)f * spf + (size_t)d.cell], 1u) != 0u) st = kBadSliceHeader;
            s_geom[0] = (int)st; s_geom[1] = d.x0; s_geom[2] = d.y0; s_geom[3] = d.sw; s_geom[4] = d.sh;
        }
        __syncthreads();
        if (s_geom[0] != 0) { flag = (uint32_t)s_geom[0]; break; }
        const int x0 = s_geom[1], y0 = s_geom[2], sw = s_geom[3], sh = s_geom[4];
        const bool stored = f >= a.first_out;
        uint8_t* out = a.dst + (size_t)(stored ? f - a.first_out : 0) * a.frame_stride + (size_t)x0 * 3u;
        for (int y = 0; y <= sh; ++y) {
            if (tid == 0) {
                if (y < sh) d.row(y);
            } else if (tid >= 64 && y > 0 && stored) {
                const int slot = (y - 1) % 3;
                const int16_t* l0 = s_lines + (size_t)(0 * 3 + slot) * a.line_stride + 1;
                const int16_t* l1 = s_lines + (size_t)(1 * 3 + slot) * a.line_stride + 1;
                const int16_t* l2 = s_lines + (size_t)(2 * 3 + slot) * a.line_stride + 1;
                uint8_t* o = out + (size_t)(y0 + y - 1) * a.pitch;
                for (int x = tid - 64; x < sw; x += 64) {
                    int g = l0[x], b = l1[x] - 256, r = l2[x] - 256;
                    g -= (b + r) >> 2;
                    b += g; r += g;
                    o[3 * x + a.ri] = (uint8_t)r; o[3 * x + 1] = (uint8_t)g; o[3 * x + a.bi] = (uint8_t)b;
                }
            }
            __syncthreads();
        }
        if (tid == 0) s_geom[0] = (int)d.finish();
        __syncthreads();
        if (s_geom[0] != 0) { flag = (uint32_t)s_geom[0]; break; }
    }
    if (flag != kOk && tid == 0) {
        atomicMax(&a.status[f], flag);
        for (int j = f + 1; j < a.n_frames && a.kind[j] != kFrameKey; ++j) atomicMax(&a.status[j], kBrokenRun);
    }
}

}  // namespace

size_t ffv1_stream_lds_bytes(int coder, int line_stride)
{
    const size_t lines = (size_t)9 * (size_t)line_stride * sizeof(int16_t);
    return 2 * (size_t)(coder ? mdvt_ffv1::kStateBytes : mdvt_ffv1::kVlcBytes) + (lines < 1024 ? 1024 : lines);
}

// static LDS of k_ffv1_stream_chain, rounded up
size_t ffv1_stream_static_lds_bytes() { return 256 * 3 + 64 + kChainThreads * 4 + 64; }

hipError_t launch_ffv1_stream_decode(const Ffv1StreamArgs& a, const Ffv1StateTables& tab, hipStream_t s)
{
    const size_t lds = ffv1_stream_lds_bytes(a.coder, a.line_stride);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_ffv1_stream_chain), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ffv1_stream_walk, dim3((a.n_frames + kWalkThreads - 1) / kWalkThreads), dim3(kWalkThreads), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ffv1_stream_chain, dim3(a.n_frames * a.nh * a.nv), dim3(kChainThreads), lds, s, a, tab);
    return hipGetLastError();
}

}  // namespace mdvt
