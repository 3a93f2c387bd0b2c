// mdvt_ffv1_stream_decode.hip -- FFV1 streams whose context state carries from frame to frame (mdvt_decode_video_stream,
// include/mdvt_ffv1_stream_decode.h): version 3, coder_type 0 (Golomb-Rice with run mode) or 1 (range coder), intra 0 or 1, RGB
// (the JPEG 2000 RCT) or 8-bit YCbCr in 4:4:4, 4:2:2 or 4:2:0.  The
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
//                         RCT of row y - 1 and stores it (not for frames before first_out): the steps of k_ffv1_dec_slice, from
//                         mdvt_ffv1_decode_common.h.  A YCbCr stream's slice is plane after plane instead: lane 0 decodes a plane
//                         row while the second wave parks the row before it (Y, Cb) in the slice's own pixels of the stored frame,
//                         or, for a row of Cr, converts its blocks to RGB there (ffv1_decode_rows_planar).
//                         A frame it has to flag ends the chain: every later frame of the run gets kBrokenRun.
//                         The workgroup of (frame 0, slice 0) also flags the frames in front of the call's first key frame.
// Every loop here is bounded by the frame's geometry, the packet's byte count or the number of frames, never by a decoded value.
#include "mdvt_ffv1_decode_common.h"

namespace mdvt {
namespace {

__global__ void __launch_bounds__(kFfv1WalkThreads) k_ffv1_stream_walk(Ffv1DecodeArgs a) { ffv1_walk_frame(a, a.kind); }

__global__ void __launch_bounds__(kFfv1DecThreads) k_ffv1_stream_chain(Ffv1DecodeArgs a, Ffv1StateTables tab)
{
    __shared__ Ffv1DecLds s;
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
    const uint32_t st_bytes = (uint32_t)state_bytes(a.coder);
    uint8_t* s_st = reinterpret_cast<uint8_t*>(s_dyn);
    int16_t* s_lines = reinterpret_cast<int16_t*>(s_st + st_bytes);
    const size_t slices = (size_t)a.n_frames * (size_t)spf;

    ffv1_fill_tables(s, tab);
    if (a.coder) {
        for (uint32_t k = tid; k < st_bytes / 4u; k += kFfv1DecThreads) s_dyn[k] = 0x80808080u;
    } else {
        VlcState* vs = reinterpret_cast<VlcState*>(s_st);
        for (int k = tid; k < 2 * kContexts; k += kFfv1DecThreads) vlc_reset(vs + k);
    }

    SliceDec<GlobalSrc, true> d;
    d.st = s_st; d.lines = s_lines; d.misc = s.misc; d.q11 = s.q11; d.stride = a.line_stride;
    int f = f0;
    uint32_t flag = kOk;                                   // why the chain ends at frame f (uniform across the workgroup)
    for (; f < a.n_frames; ++f) {
        const uint32_t kind = a.kind[f];                   // (written by the walk alone: the same word for every thread)
        if (f > f0 && kind == kFrameKey) break;            // the next run's workgroup takes over
        if (kind == kFrameBad) { flag = kBadPacket; break; }
        const size_t i = (size_t)f * spf + (size_t)si;
        const uint32_t off = a.table[i], len = a.table[slices + i];
        const uint8_t* data = a.packets + a.offsets[f] + off;
        __syncthreads();                                   // the last frame's rows are stored; the tables and the state are set
        if (!ffv1_prepare_slice(a, s, s_lines, data, len)) { flag = kCrcMismatch; break; }
        if (tid == 0) {
            const uint32_t st = ffv1_begin_slice(d, a, s, data, len, si);          // (d.key: the walk has read that bit already)
            ffv1_claim_cell(d, a, s, f, st);
        }
        __syncthreads();
        if (s.geom[0] != 0) { flag = (uint32_t)s.geom[0]; break; }
        const bool stored = f >= a.first_out;
        uint8_t* frame = a.dst + (size_t)(stored ? f - a.first_out : 0) * a.frame_stride;
        if (a.planar) ffv1_decode_rows_planar(d, a, s, s_lines, frame, stored);
        else ffv1_decode_rows(d, a, s, s_lines, frame, stored);
        if (tid == 0) s.geom[0] = (int)d.finish();
        __syncthreads();
        if (s.geom[0] != 0) { flag = (uint32_t)s.geom[0]; break; }
    }
    if (flag != kOk && tid == 0) {
        atomicMax(&a.status[f], flag);
        for (int j = f + 1; j < a.n_frames && a.kind[j] != kFrameKey; ++j) atomicMax(&a.status[j], kBrokenRun);
    }
}

}  // namespace

size_t ffv1_stream_lds_bytes(int coder, int line_stride) { return mdvt_ffv1::state_bytes(coder) + ffv1_row_slots_bytes(line_stride); }

hipError_t launch_ffv1_stream_decode(const Ffv1DecodeArgs& a, const Ffv1StateTables& tab, hipStream_t s)
{
    return ffv1_launch(k_ffv1_stream_walk, k_ffv1_stream_chain, ffv1_stream_lds_bytes(a.coder, a.line_stride), a, tab, s);
}

}  // namespace mdvt
