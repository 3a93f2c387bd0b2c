// mdvt_ffv1_decode.hip -- FFV1 decoding of packets in device memory (mdvt_decode_video_frames, include/mdvt_ffv1_decode.h): the
// bytes mdvt_video_read (csrc_host/mdvt_video.cpp) writes for the same packet, for the stream class the project's own writer
// makes (version 3, range coder with the default state table, key frames only, RGB, 8 bits, the default 666 contexts, slices
// with or without their CRC).  Every slice of every frame is an independent range decoder: the mirror image of k_ffv1_code.
// The steps of one slice are mdvt_ffv1_decode_common.h's, shared with the stream decoder; here is what a pass of key frames adds:
// one workgroup per slice of one frame, the context state in static LDS, and flags raised with atomicMax.
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
#include "mdvt_ffv1_decode_common.h"

namespace mdvt {
namespace {

__global__ void __launch_bounds__(kFfv1WalkThreads) k_ffv1_dec_walk(Ffv1DecodeArgs a) { ffv1_walk_frame(a, nullptr); }

__global__ void __launch_bounds__(kFfv1DecThreads) k_ffv1_dec_slice(Ffv1DecodeArgs a, Ffv1StateTables tab)
{
    __shared__ uint32_t s_st[2 * kStateBytes / 4];
    __shared__ Ffv1DecLds s;
    extern __shared__ int16_t s_lines[];                   // 3 planes x 3 slots x line_stride samples; the CRC table before that
    const int tid = (int)threadIdx.x;
    const int spf = a.nh * a.nv;
    const int i = (int)blockIdx.x;                         // slice of the pass
    const int f = i / spf, si = i - f * spf;
    if (tid == 0) s.geom[0] = (int)a.status[f];            // (one read for the workgroup: other slices of the frame may flag it meanwhile)
    __syncthreads();
    if (s.geom[0] != 0) return;                            // the walk refused the packet, or a slice before this one flagged the frame
    const size_t slices = (size_t)a.n_frames * (size_t)spf;
    const uint32_t off = a.table[i], len = a.table[slices + i];
    const uint8_t* data = a.packets + a.offsets[f] + off;

    for (int k = tid; k < 2 * kStateBytes / 4; k += kFfv1DecThreads) s_st[k] = 0x80808080u;
    ffv1_fill_tables(s, tab);
    if (!ffv1_prepare_slice(a, s, s_lines, data, len)) {
        if (tid == 0) atomicMax(&a.status[f], kCrcMismatch);
        return;
    }

    SliceDec<GlobalSrc> d;
    if (tid == 0) {
        d.st = reinterpret_cast<uint8_t*>(s_st); d.lines = s_lines; d.misc = s.misc; d.q11 = s.q11; d.stride = a.line_stride;
        uint32_t st = ffv1_begin_slice(d, a, s, data, len, si);
        if (st == kOk && si == 0 && !d.key) st = kBadSliceHeader;                  // not a key frame: outside this decoder's class
        ffv1_claim_cell(d, a, s, f, st);
    }
    __syncthreads();
    if (s.geom[0] != 0) {
        if (tid == 0) atomicMax(&a.status[f], (uint32_t)s.geom[0]);
        return;
    }
    ffv1_decode_rows(d, a, s, s_lines, a.dst + (size_t)f * a.frame_stride, true);
    if (tid == 0) {
        const uint32_t st = d.finish();
        if (st != kOk) atomicMax(&a.status[f], st);
    }
}

}  // namespace

size_t ffv1_decode_lds_bytes(int line_stride) { return ffv1_row_slots_bytes(line_stride); }

// Ffv1DecLds, rounded up
size_t ffv1_decode_static_lds_bytes() { return 256 * 3 + 64 + kFfv1DecThreads * 4 + 64; }
static_assert(sizeof(Ffv1DecLds) <= 256 * 3 + 64 + kFfv1DecThreads * 4 + 64, "the rounded-up figure no longer covers the struct");

hipError_t launch_ffv1_decode(const Ffv1DecodeArgs& a, const Ffv1StateTables& tab, hipStream_t s)
{
    return ffv1_launch(k_ffv1_dec_walk, k_ffv1_dec_slice, ffv1_decode_lds_bytes(a.line_stride), a, tab, s);
}

}  // namespace mdvt
