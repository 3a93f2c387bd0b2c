/* mdvt_ffv1_stream_decode.h -- FFV1 streams with inter frames and Golomb-Rice coding, decoded on the device.
 *
 * mdvt_decode_video_frames (include/mdvt_ffv1_decode.h) reads the class this project's default writer makes: range coder, every
 * frame a key frame.  The files FFmpeg and OpenCV write by default are another class: version 3, coder_type 0 (Golomb-Rice with run
 * mode), intra = 0, a key frame every 12 frames -- the reference's x_depth.mkv (save_depth_video) and the scene clips of
 * movie_2_3D.py.  There the context state of a slice carries from frame to frame up to the next key frame, so the unit of parallel
 * work is (key-frame run, slice), not (frame, slice).  This header's call decodes both classes that way; it is held to
 * mdvt_video_read and to the independent restatement ffv1_ref.py, not to a file FFmpeg wrote (that parity stays unpinned).
 *
 * State is not carried from one call to the next: every call starts without a key frame, and the frames in front of the first key
 * frame it is given are flagged.  A caller that wants frames a .. b passes the packets from the last key frame at or before a and
 * says with first_out where the stored frames begin.
 */
#ifndef MDVT_FFV1_STREAM_DECODE_H
#define MDVT_FFV1_STREAM_DECODE_H

#include <stddef.h>
#include <stdint.h>

#include "mdvt.h"
#include "mdvt_ffv1_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Status words of this call, after MDVT_FFV1_DECODED .. MDVT_FFV1_BAD_PACKET (0 .. 4) of mdvt_ffv1_decode.h. */
#define MDVT_FFV1_NO_KEY_FRAME 5u     /* no key frame at or before this frame inside the call */
#define MDVT_FFV1_BROKEN_RUN 6u       /* an earlier frame of this key-frame run was flagged: this frame's context state is unknown */

/* Decodes n_packets consecutive frames of one FFV1 stream whose packets lie in device memory (as for mdvt_decode_video_frames:
 * packet k is d_sizes[k] bytes at d_packets + d_offsets[k], inside [d_packets, d_packets + packets_bytes)).  Frames
 * first_out .. n_packets - 1 are stored, frame k at d_dst + (k - first_out) * frame_stride + row * pitch, 3 bytes per pixel
 * (order 0: R, G, B; 1: B, G, R).  The frames before first_out are decoded for their context state alone; nothing is stored for
 * them.  A stored frame whose status word is 0 is byte for byte what mdvt_video_read writes when it reads the same packets in
 * order from the run's key frame.  The call only enqueues on `stream`; the key frames' positions are found on the device, nothing
 * is read back.
 *
 * h_config / config_size: the configuration record in host memory.  Decoded: version 3 (any micro version), coder_type 0
 * (Golomb-Rice) or 1 (range coder, default state-transition table), intra 0 or 1, 8 bits, no alpha plane, one
 * quantisation-table set equal to the default 666-context set without initial states, ec 0 or 1, 1 to 1024 slices per frame;
 * colorspace_type 1 (RGB, the JPEG 2000 RCT) or 0 (YCbCr) with chroma_planes 1 and log2 chroma subsampling (0, 0), (1, 0) or
 * (1, 1): yuv444p, yuv422p, yuv420p.  Any other record returns MDVT_ERR_UNSUPPORTED with the reason (it names the field) before
 * anything is launched or written; so does a YCbCr record whose slice grid puts a slice origin off the chroma grid on this frame
 * size (x0 not a multiple of 2^hs, or y0 of 2^vs: the reason names the grid), which the host reader refuses as well.  The old
 * cases of mdvt_decode_video_frames and a first_out outside [0, n_packets) return MDVT_ERR_INVALID_ARG (frame_stride matters when
 * more than one frame is stored).
 *
 * d_status[k] (n_packets words, all written): 0, one of the words of mdvt_ffv1_decode.h for the frame that is itself at fault, or
 *   MDVT_FFV1_NO_KEY_FRAME   frame k has no key frame at or before it inside the call;
 *   MDVT_FFV1_BROKEN_RUN     a frame between the run's key frame and k was flagged.  A flagged frame flags every later frame up
 *                            to the next key frame; a frame whose packet is refused (MDVT_FFV1_BAD_PACKET) counts as an inter frame.
 * The largest word wins.  A flagged frame's bytes are unspecified inside its own rows: decode its run on the host.  As for
 * mdvt_decode_video_frames, a frame whose slice headers do not place exactly one slice on every cell is flagged.  The host reader
 * has no overread check on the Golomb-Rice side (bits past a slice's end read as zero): such a slice decodes to the host's bytes
 * with status 0 here too.  Nothing read from a packet steers a loop or an address.
 *
 * A YCbCr stream's planes are decoded exactly (RFC 9043: Y, then Cb, then Cr, 8-bit samples, the run index restarting at each
 * plane) and converted to R, G, B as include/mdvt_video.h decrees it -- BT.601 limited range, chroma replicated; this project's
 * formula, not an observation of swscale or cv2.  The planes of a slice arrive one after another, so its luma and Cb rows wait
 * inside the slice's own pixels of the stored frame until their Cr row converts them: nothing outside the footprint below is
 * touched, every byte inside it is finally the frame's, and frames before first_out still store nothing.
 *
 * Footprint: the first 3 * width bytes of each row of each stored frame, and n_packets status words; nothing else of the caller's.
 * The result does not depend on bytes outside the packets.  Workspace (12 bytes per slice and 4 per frame of the call) comes from
 * the context's pool; a call whose workspace passes mdvt_config.workspace_mib returns MDVT_ERR_UNSUPPORTED: a run cannot be split
 * into passes, so split the call at a key frame.
 *
 * Cost: one workgroup decodes one slice through all the frames of one key-frame run, serially, so a call runs as long as its
 * longest chain -- (frames of the run inside the call) x (samples of one slice) -- and uses as many workgroups as it has
 * (runs) x (slices).  Nothing here bounds that: a stream with few slices per frame and long runs keeps a few lanes busy for a
 * long time (a 1080p colour stream in 2 x 2 slices decodes at about 4 frames per second, profiles/r12_ffv1_stream_decoder.md).
 * Give such a stream to the host reader. */
int mdvt_decode_video_stream(mdvt_ctx* ctx, int width, int height, const uint8_t* h_config, size_t config_size,
                             const uint8_t* d_packets, uint64_t packets_bytes, const uint64_t* d_offsets, const uint32_t* d_sizes,
                             int n_packets, int first_out, uint8_t* d_dst, size_t pitch, size_t frame_stride, int order,
                             uint32_t* d_status, void* stream);

/* NULL when mdvt_decode_video_stream decodes streams with this configuration record (host memory), else the reason as a static
 * string that names the field.  Needs no device and no context. */
const char* mdvt_ffv1_stream_decode_supported(const uint8_t* h_config, size_t config_size);

/* Host: the key-frame bit of a packet in host memory, the first range-coded bit (1 key frame, 0 inter frame; -1 for a packet of
 * fewer than 3 bytes, which no reader accepts).  Needs no device and no context. */
int mdvt_ffv1_packet_is_key(const uint8_t* h_packet, size_t size);

#ifdef __cplusplus
}
#endif
#endif
