// mdvt_ffv1_decode_common.h -- what the two FFV1 decode kernels share on the device: k_ffv1_dec_slice (mdvt_ffv1_decode.hip: one
// slice of one key frame per workgroup) and k_ffv1_stream_chain (mdvt_ffv1_stream_decode.hip: one slice through the frames of a
// key-frame run per workgroup).  The byte sources, the per-frame walk, and the steps a workgroup of two waves takes for one slice
// of one frame: the CRC check, lane 0's begin with the cell claim, and the row loop in which lane 0 decodes row y while the second
// wave undoes the RCT of row y - 1 and stores it.  One barrier per row.  What differs stays in the two files: which slices a
// workgroup takes, where the context state lives and how a flag reaches the status words.
// Every loop here is bounded by the frame's geometry or the packet's byte count, never by a value decoded from the packet.
#pragma once

#include "mdvt_internal.h"
#include "mdvt_ffv1_core.h"

namespace mdvt {
namespace {

using namespace mdvt_ffv1;

constexpr int kFfv1DecThreads = 128;                       // a slice's workgroup: lane 0 decodes, the second wave stores
constexpr int kFfv1WalkThreads = 64;

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

// the static LDS of a slice's workgroup (the context state and the row slots are the kernels' own)
struct Ffv1DecLds {
    uint16_t next[256];                                    // zero_state | one_state << 8
    uint8_t misc[64];
    int8_t q11[256];
    uint32_t part[kFfv1DecThreads];
    int geom[5];                                           // status, x0, y0, sw, sh
};

// One thread per frame: the frame's packet is checked against the packet buffer, and its slice table (offset and payload bytes of
// each slice) is found by walking back from the packet's end.  Writes the frame's status word, 0 or kBadPacket -- no decoder then
// touches the packet --, and where `kind_of` is not null (the stream call's a.kind), the frame's kind: its key-frame bit as the range
// decoder decides it.
__device__ __forceinline__ void ffv1_walk_frame(const Ffv1DecodeArgs& a, uint32_t* kind_of)
{
    const int f = (int)(blockIdx.x * kFfv1WalkThreads + threadIdx.x);
    if (f >= a.n_frames) return;
    const int spf = a.nh * a.nv;
    const unsigned long long off = a.offsets[f];
    const uint32_t size = a.sizes[f];
    uint32_t st = kBadPacket, kind = kFrameBad;
    if (off <= a.packets_bytes && size <= a.packets_bytes - off) {
        const size_t slices = (size_t)a.n_frames * (size_t)spf;
        const uint8_t* pkt = a.packets + off;
        st = walk_slices(PacketByte{pkt}, size, spf, a.ec, a.table + (size_t)f * spf, a.table + slices + (size_t)f * spf);
        if (kind_of && st == kOk) kind = key_frame_bit(pkt[0], pkt[1]) ? kFrameKey : kFrameInter;      // (size >= 3: walk_slices)
    }
    a.status[f] = st;
    if (kind_of) kind_of[f] = kind;
}

__device__ __forceinline__ void ffv1_fill_tables(Ffv1DecLds& s, const Ffv1StateTables& tab)
{
    for (int k = (int)threadIdx.x; k < 256; k += kFfv1DecThreads) {
        s.next[k] = (uint16_t)(tab.zero[k] | (tab.one[k] << 8));
        s.q11[k] = (int8_t)quant11(k);
    }
}

// The workgroup, before lane 0 begins a slice of len payload bytes at `data`.  With ec it verifies the slice's CRC-32: contiguous
// chunks, each chunk's CRC shifted over the bytes behind it, as k_ffv1_emit makes it.  The CRC table borrows the row slots' place.
// Then the row slots are zeroed.  -> false for a CRC mismatch (the slice is not to be decoded); the same value in every thread
__device__ __forceinline__ bool ffv1_prepare_slice(const Ffv1DecodeArgs& a, Ffv1DecLds& s, int16_t* s_lines, const uint8_t* data, uint32_t len)
{
    const int tid = (int)threadIdx.x;
    if (a.ec) {
        const uint32_t n = len + 8u;                       // payload, size bytes, error byte and parity: the CRC of all of it is zero
        uint32_t* s_crc = reinterpret_cast<uint32_t*>(s_lines);
        for (int k = tid; k < 256; k += kFfv1DecThreads) s_crc[k] = crc_table_entry((uint32_t)k);
        __syncthreads();
        const uint32_t per = (n + kFfv1DecThreads - 1) / kFfv1DecThreads;
        const uint32_t b0 = per * (uint32_t)tid < n ? per * (uint32_t)tid : n;
        const uint32_t b1 = b0 + per < n ? b0 + per : n;
        uint32_t crc = 0;
        for (uint32_t k = b0; k < b1; ++k) crc = (crc << 8) ^ s_crc[(crc >> 24) ^ data[k]];
        s.part[tid] = crc_shift(crc, n - b1);
        __syncthreads();
        if (tid == 0) {
            uint32_t all = 0;
            for (int k = 0; k < kFfv1DecThreads; ++k) all ^= s.part[k];
            s.geom[0] = all ? (int)kCrcMismatch : 0;
        }
        __syncthreads();
        if (s.geom[0] != 0) return false;
    }
    for (int k = tid; k < 9 * a.line_stride; k += kFfv1DecThreads) s_lines[k] = 0;
    __syncthreads();
    return true;
}

// Lane 0: the slice's header (SliceDec::begin) from its len payload bytes at `data`; si: the slice's place in the packet
template <class Dec>
__device__ __forceinline__ uint32_t ffv1_begin_slice(Dec& d, const Ffv1DecodeArgs& a, const Ffv1DecLds& s, const uint8_t* data, uint32_t len, int si)
{
    const uint32_t avail = len + (a.ec ? 8u : 3u);         // [data, data + avail) lies inside the packet (the walk)
    GlobalSrc src;
    src.p = data; src.avail = avail; src.wbase = 0xFFFFFF00u; src.w = 0;
    return d.begin(src, avail, len, si == 0, a.coder, a.micro, a.W, a.H, a.nh, a.nv, s.next, a.planar, a.hs, a.vs);
}

// Lane 0, with begin's status: every slice of frame f claims its cell before it stores, so two slices never write the same pixels,
// and as there are as many slices as cells, a frame without a flag has every cell written.  Publishes the status and the slice's
// rectangle for the workgroup (s.geom, read behind a barrier).
template <class Dec>
__device__ __forceinline__ void ffv1_claim_cell(const Dec& d, const Ffv1DecodeArgs& a, Ffv1DecLds& s, int f, uint32_t st)
{
    if (st == kOk && atomicExch(&a.claims[(size_t)f * (size_t)(a.nh * a.nv) + (size_t)d.cell], 1u) != 0u) st = kBadSliceHeader;
    s.geom[0] = (int)st; s.geom[1] = d.x0; s.geom[2] = d.y0; s.geom[3] = d.sw; s.geom[4] = d.sh;
}

// The workgroup: the rows of the slice whose rectangle is in s.geom.  Lane 0 decodes row y; meanwhile the second wave undoes the RCT
// of row y - 1 and stores it in the frame at `frame` -- unless !stored: a frame decoded for its context state alone.
template <class Dec>
__device__ __forceinline__ void ffv1_decode_rows(Dec& d, const Ffv1DecodeArgs& a, const Ffv1DecLds& s, const int16_t* s_lines, uint8_t* frame, bool stored)
{
    const int tid = (int)threadIdx.x;
    const int x0 = s.geom[1], y0 = s.geom[2], sw = s.geom[3], sh = s.geom[4];
    uint8_t* out = frame + (size_t)x0 * 3u;
    for (int y = 0; y <= sh; ++y) {
        if (tid == 0) {
            if (y < sh) d.row(y);
        } else if (tid >= 64 && y > 0 && stored) {
            const int slot = (y - 1) % 3;
            const int16_t* l0 = s_lines + (size_t)(0 * 3 + slot) * a.line_stride + 1;
            const int16_t* l1 = s_lines + (size_t)(1 * 3 + slot) * a.line_stride + 1;
            const int16_t* l2 = s_lines + (size_t)(2 * 3 + slot) * a.line_stride + 1;
            uint8_t* o = out + (size_t)(y0 + y - 1) * a.pitch;
            for (int x = tid - 64; x < sw; x += 64) store_rct_pixel(l0[x], l1[x], l2[x], o, 3 * x + a.ri, 3 * x + 1, 3 * x + a.bi);
        }
        __syncthreads();
    }
}

// The workgroup, for a slice of a YCbCr stream (a.planar): the slice's plane rows in coding order -- Y's, then Cb's, then Cr's.  Lane 0
// decodes plane row r while the second wave takes plane row r - 1 from its slot to the frame (planar_store_row): Y and Cb wait in
// the slice's own pixels, a row of Cr converts its blocks to RGB.  The barrier between two steps orders the second wave's stores of
// one step before its loads of a later one.  Nothing is stored for a frame decoded for its context state alone.
template <class Dec>
__device__ __forceinline__ void ffv1_decode_rows_planar(Dec& d, const Ffv1DecodeArgs& a, const Ffv1DecLds& s, const int16_t* s_lines, uint8_t* frame,
                                                        bool stored)
{
    const int tid = (int)threadIdx.x;
    const int x0 = s.geom[1], y0 = s.geom[2], sw = s.geom[3], sh = s.geom[4];
    const int csw = (sw + (1 << a.hs) - 1) >> a.hs, csh = (sh + (1 << a.vs) - 1) >> a.vs;
    const int total = sh + 2 * csh;
    uint8_t* rect = frame + (size_t)y0 * a.pitch + (size_t)x0 * 3u;
    for (int r = 0; r <= total; ++r) {
        if (tid == 0) {
            if (r < total) d.plane_row(r < sh ? 0 : r < sh + csh ? 1 : 2, r < sh ? r : r < sh + csh ? r - sh : r - sh - csh);
        } else if (tid >= 64 && r > 0 && stored) {
            const int q = r - 1;
            const int p = q < sh ? 0 : q < sh + csh ? 1 : 2, y = q < sh ? q : q < sh + csh ? q - sh : q - sh - csh;
            planar_store_row(s_lines + (size_t)(p * 3 + y % 3) * a.line_stride + 1, p, y, rect, a.pitch, sw, sh, csw, a.hs, a.vs, a.ri, a.bi,
                             tid - 64, 64);
        }
        __syncthreads();
    }
}

// the row slots' bytes in LDS (the CRC table borrows their place)
inline size_t ffv1_row_slots_bytes(int line_stride)
{
    const size_t lines = (size_t)9 * (size_t)line_stride * sizeof(int16_t);
    return lines < 1024 ? 1024 : lines;
}

// the two launches of a pass: the walk, then one workgroup per (frame, slice) with `lds` bytes of dynamic LDS
inline hipError_t ffv1_launch(void (*walk)(Ffv1DecodeArgs), void (*slice)(Ffv1DecodeArgs, Ffv1StateTables), size_t lds, const Ffv1DecodeArgs& a,
                              const Ffv1StateTables& tab, hipStream_t s)
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(slice), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(walk, dim3((a.n_frames + kFfv1WalkThreads - 1) / kFfv1WalkThreads), dim3(kFfv1WalkThreads), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(slice, dim3(a.n_frames * a.nh * a.nv), dim3(kFfv1DecThreads), lds, s, a, tab);
    return hipGetLastError();
}

}  // namespace
}  // namespace mdvt
