/* mdvt_ffv1_decode.h -- FFV1 decoding on the device: the one entry point of libmdvt_hip.so that is declared outside include/mdvt.h.
 *
 * The device twin of mdvt_video_read (include/mdvt_video.h) for the streams this project's writer makes, as
 * mdvt_encode_video_frames (include/mdvt.h) is the twin of mdvt_video_write.  It replaces the reference's cv2.VideoCapture reads
 * of its own outputs (stereo_rerender.py:326-341, 489-509; basic_nomal_infill.py:129-171) where those files were written by this
 * project: the packets are copied to the device as stored and the raw frames never exist on the host.
 */
#ifndef MDVT_FFV1_DECODE_H
#define MDVT_FFV1_DECODE_H

#include <stddef.h>
#include <stdint.h>

#include "mdvt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-frame status words. */
#define MDVT_FFV1_DECODED 0u          /* the frame's bytes are those of mdvt_video_read */
#define MDVT_FFV1_CRC_MISMATCH 1u     /* a slice's CRC-32 parity fails (ec streams); the slice was not decoded */
#define MDVT_FFV1_BAD_SLICE_HEADER 2u /* not a key frame, a malformed slice header, or slices that do not tile the frame */
#define MDVT_FFV1_DAMAGED 3u          /* the bitstream ran dry beyond the host reader's allowance, or a symbol is malformed */
#define MDVT_FFV1_BAD_PACKET 4u       /* the slice sizes do not add up to the packet, or the packet passes the packet buffer */

/* Decodes n_frames FFV1 packets that lie in device memory -- packet k is d_sizes[k] bytes at d_packets + d_offsets[k], all inside
 * [d_packets, d_packets + packets_bytes) -- into n_frames frames of `height` rows of `width` pixels of 3 bytes (order 0: R, G, B;
 * 1: B, G, R) at d_dst + k * frame_stride + row * pitch: byte for byte what mdvt_video_read writes for the same packet.  The call
 * only enqueues on `stream` (a hipStream_t; NULL = the default stream); width and height are those of the video, independent of the
 * size the context renders at.
 *
 * h_config / config_size: the stream's configuration record in host memory (mdvt_video_config_record), parsed here.  The device
 * decodes: version 3 (any micro version), coder_type 1 (range coder, default state-transition table), every frame a key frame
 * (intra = 1), RGB colour space, 8 bits, no alpha plane, one quantisation-table set equal to the default 666-context set without
 * initial states, 1 to 1024 slices per frame, with and without the slices' CRC-32 (ec 1 and 0).  Any other record returns
 * MDVT_ERR_UNSUPPORTED with the reason (it names the field) in mdvt_last_error, before anything is launched or written: read such
 * a stream with mdvt_video_read.  NULL buffers, a pitch below 3 * width, a frame_stride below height * pitch (n_frames > 1),
 * n_frames < 1 or an unknown order return MDVT_ERR_INVALID_ARG.
 *
 * d_status[k] (n_frames words, all written): MDVT_FFV1_DECODED, or the reason frame k was not decoded.  The packet's structure and
 * (ec streams) every slice's CRC are verified on the device before a range decoder reads a byte; nothing read from a packet
 * steers a loop or an address, so a malformed packet ends in a status word.  A flagged frame's bytes are unspecified (inside
 * its own rows): decode that packet on the host (mdvt_ffv1_decode_frame / mdvt_video_read), which gives the host's own error.
 * The frames the host reader refuses are flagged.  Two kinds of frame the host reader accepts are flagged as well, because they
 * are outside the class above: a frame whose key-frame bit is clear, and a frame whose slice headers do not place exactly one
 * slice on every cell of the slice grid (the host reader decodes such slices over each other).
 *
 * Footprint: exactly the first 3 * width bytes of each of the `height` rows of each of the n_frames frames of d_dst, and n_frames
 * words of d_status; nothing else of the caller's.  The result does not depend on bytes outside the packets.  Workspace (12 bytes
 * per slice of a pass) comes from the context's pool and is bounded by mdvt_config.workspace_mib, like the encoder's. */
int mdvt_decode_video_frames(mdvt_ctx* ctx, int width, int height, const uint8_t* h_config, size_t config_size,
                             const uint8_t* d_packets, uint64_t packets_bytes, const uint64_t* d_offsets, const uint32_t* d_sizes,
                             int n_frames, uint8_t* d_dst, size_t pitch, size_t frame_stride, int order, uint32_t* d_status,
                             void* stream);

/* NULL when mdvt_decode_video_frames decodes streams with this configuration record (host memory), else the reason as a static
 * string that names the field.  Needs no device and no context. */
const char* mdvt_ffv1_decode_supported(const uint8_t* h_config, size_t config_size);

#ifdef __cplusplus
}
#endif
#endif
