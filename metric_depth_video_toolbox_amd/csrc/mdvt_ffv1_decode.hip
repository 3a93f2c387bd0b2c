// mdvt_ffv1_decode.hip -- FFV1 decoding of packets in device memory (mdvt_decode_video_frames, include/mdvt_ffv1_decode.h): the
// bytes mdvt_video_read (csrc_host/mdvt_video.cpp) writes for the same packet, for the stream class the project's own writer
// makes (version 3, range coder with the default state table, key frames only, RGB, 8 bits, the default 666 contexts, slices
// with or without their CRC).  Every slice of every frame is an independent range decoder: the mirror image of k_ffv1_code.
//
// Two launches per pass:
//   k_ffv1_dec_walk    one thread per frame: the frame's packet is checked against the packet buffer, and its slice table
//                      (offset and payload bytes of each slice) is found by walking back from the packet's end, every entry
//                      checked against the packet as the host reader checks it.  Writes the frame's status word: 0, or
//                      kBadPacket -- no decoder then touches the packet.
//   k_ffv1_dec_slice   one workgroup of two waves per slice.  The two context-state sets (2 x 666 x 32 B) live in LDS, as do
//                      three row slots per RCT plane.  With ec the whole workgroup first verifies the slice's CRC-32 (contiguous
//                      chunks, each chunk's CRC shifted over the bytes behind it, as k_ffv1_emit makes it); a slice that fails
//                      is not decoded.  Lane 0 of the first wave then reads the key-frame bit and the slice header, claims the
//                      slice's cell of the frame (a cell claimed twice flags the frame before anything is stored), and decodes
//                      row by row, plane by plane; while it decodes row y the second wave undoes the RCT of row y - 1 and
//                      stores it.  One barrier per row.
// The decoder itself (mdvt_ffv1_core.h) is plain C++ shared with a host test program; every loop in it and here is bounded by
// the frame's geometry or the packet's byte count, never by a value decoded from the packet.
#include "mdvt_internal.h"
#include "mdvt_ffv1_core.h"

namespace mdvt {
namespace {

using namespace mdvt_ffv1;

constexpr int kDecThreads = 128;
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

__global__ void __launch_bounds__(kWalkThreads) k_ffv1_dec_walk(Ffv1DecodeArgs a)
{
    const int f = (int)(blockIdx.x * kWalkThreads + threadIdx.x);
    if (f >= a.n_frames) return;
    const int spf = a.nh * a.nv;
    const unsigned long long off = a.offsets[f];
    const uint32_t size = a.sizes[f];
    uint32_t st = kBadPacket;
    if (off <= a.packets_bytes && size <= a.packets_bytes - off) {
        const size_t slices = (size_t)a.n_frames * (size_t)spf;
        st = walk_slices(PacketByte{a.packets + off}, size, spf, a.ec, a.table + (size_t)f * spf, a.table + slices + (size_t)f * spf);
    }
    a.status[f] = st;
}

__global__ void __launch_bounds__(kDecThreads) k_ffv1_dec_slice(Ffv1DecodeArgs a, Ffv1StateTables tab)
{
    __shared__ uint8_t s_st[2 * kStateBytes];
    __shared__ uint16_t s_next[256];                       // zero_state | one_state << 8
    __shared__ uint8_t s_misc[64];
    __shared__ int8_t s_q11[256];
    __shared__ uint32_t s_part[kDecThreads];
    __shared__ int s_geom[5];                              // status, x0, y0, sw, sh
    extern __shared__ int16_t s_lines[];                   // 3 planes x 3 slots x line_stride samples; the CRC table before that
    const int tid = (int)threadIdx.x;
    const int spf = a.nh * a.nv;
    const int i = (int)blockIdx.x;                         // slice of the pass
    const int f = i / spf, si = i - f * spf;
    if (tid == 0) s_geom[0] = (int)a.status[f];            // (one read for the workgroup: other slices of the frame may flag it meanwhile)
    __syncthreads();
    if (s_geom[0] != 0) return;                            // the walk refused the packet, or a slice before this one flagged the frame
    const size_t slices = (size_t)a.n_frames * (size_t)spf;
    const uint32_t off = a.table[i], len = a.table[slices + i];
    const uint32_t trailer = a.ec ? 8u : 3u;
    const uint8_t* data = a.packets + a.offsets[f] + off;  // [data, data + len + trailer) lies inside the packet (k_ffv1_dec_walk)

    uint32_t* st32 = reinterpret_cast<uint32_t*>(s_st);
    for (int k = tid; k < 2 * kStateBytes / 4; k += kDecThreads) st32[k] = 0x80808080u;
    for (int k = tid; k < 256; k += kDecThreads) { s_next[k] = (uint16_t)(tab.zero[k] | (tab.one[k] << 8)); s_q11[k] = (int8_t)quant11(k); }
    uint32_t* s_crc = reinterpret_cast<uint32_t*>(s_lines);
    if (a.ec) {
        for (int k = tid; k < 256; k += kDecThreads) s_crc[k] = crc_table_entry((uint32_t)k);
        __syncthreads();
        const uint32_t n = len + trailer;                  // payload, size bytes, error byte and parity: the CRC of all of it is zero
        const uint32_t per = (n + kDecThreads - 1) / kDecThreads;
        const uint32_t b0 = per * (uint32_t)tid < n ? per * (uint32_t)tid : n;
        const uint32_t b1 = b0 + per < n ? b0 + per : n;
        uint32_t crc = 0;
        for (uint32_t k = b0; k < b1; ++k) crc = (crc << 8) ^ s_crc[(crc >> 24) ^ data[k]];
        s_part[tid] = crc_shift(crc, n - b1);
        __syncthreads();
        if (tid == 0) {
            uint32_t all = 0;
            for (int k = 0; k < kDecThreads; ++k) all ^= s_part[k];
            s_geom[0] = all ? (int)kCrcMismatch : 0;
        }
        __syncthreads();
        if (s_geom[0] != 0) {
            if (tid == 0) atomicMax(&a.status[f], kCrcMismatch);
            return;
        }
    }
    for (int k = tid; k < 9 * a.line_stride; k += kDecThreads) s_lines[k] = 0;
    __syncthreads();

    SliceDec<GlobalSrc> d;
    if (tid == 0) {
        d.st = s_st; d.lines = s_lines; d.misc = s_misc; d.q11 = s_q11; d.stride = a.line_stride;
        GlobalSrc src;
        src.p = data; src.avail = len + trailer; src.wbase = 0xFFFFFF00u; src.w = 0;
        uint32_t st = d.begin(src, len + trailer, len, si == 0, a.W, a.H, a.nh, a.nv, s_next);
        // every slice of the frame claims its cell before it stores: two slices never write the same pixels, and as there are as
        // many slices as cells, a frame without a flag has every cell written
        if (st == kOk && atomicExch(&a.claims[(size_t)f * spf + (size_t)d.cell], 1u) != 0u) st = kBadSliceHeader;
        s_geom[0] = (int)st; s_geom[1] = d.x0; s_geom[2] = d.y0; s_geom[3] = d.sw; s_geom[4] = d.sh;
    }
    __syncthreads();
    if (s_geom[0] != 0) {
        if (tid == 0) atomicMax(&a.status[f], (uint32_t)s_geom[0]);
        return;
    }
    const int x0 = s_geom[1], y0 = s_geom[2], sw = s_geom[3], sh = s_geom[4];
    uint8_t* out = a.dst + (size_t)f * a.frame_stride + (size_t)x0 * 3u;
    for (int y = 0; y <= sh; ++y) {
        if (tid == 0) {
            if (y < sh) d.row(y);
        } else if (tid >= 64 && y > 0) {
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
    if (tid == 0) {
        const uint32_t st = d.finish();
        if (st != kOk) atomicMax(&a.status[f], st);
    }
}

}  // namespace

size_t ffv1_decode_lds_bytes(int line_stride)
{
    const size_t lines = (size_t)9 * (size_t)line_stride * sizeof(int16_t);
    return lines < 1024 ? 1024 : lines;                    // (the CRC table borrows the rows' place)
}

// static LDS of k_ffv1_dec_slice, rounded up: what is left of a CU's 160 KiB bounds the widest slice
size_t ffv1_decode_static_lds_bytes() { return 2 * mdvt_ffv1::kStateBytes + 256 * 3 + 64 + kDecThreads * 4 + 64; }

hipError_t launch_ffv1_decode(const Ffv1DecodeArgs& a, const Ffv1StateTables& tab, hipStream_t s)
{
    const size_t lds = ffv1_decode_lds_bytes(a.line_stride);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_ffv1_dec_slice), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ffv1_dec_walk, dim3((a.n_frames + kWalkThreads - 1) / kWalkThreads), dim3(kWalkThreads), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ffv1_dec_slice, dim3(a.n_frames * a.nh * a.nv), dim3(kDecThreads), lds, s, a, tab);
    return hipGetLastError();
}

}  // namespace mdvt
