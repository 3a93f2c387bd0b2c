/*
 * mdvt_video.h -- C ABI of libmdvt_video.so: the on-disk format either side of the stereo-rerender path
 * (SURVEY.md 8f rank 2): FFV1 video in a Matroska container, as OpenCV's VideoWriter / VideoCapture produce and consume it
 * for the reference.  Host code only (C++17, no GPU, no third-party library): FFmpeg / OpenCV are absent from the image,
 * so both directions are written from the published specifications -- FFV1: RFC 9043 (versions 0, 1 and 3; range coder with
 * the default or a custom state-transition table and Golomb-Rice; the JPEG 2000 RCT "RGB" colour space at 8 bits with or
 * without alpha, and YCbCr at 8 bits in 4:4:4, 4:2:2 and 4:2:0; slices with CRC-32 parities); Matroska: RFC 9559 / EBML
 * RFC 8794 (the subset one video track needs).
 *
 * YCbCr streams (colorspace_type 0, chroma_planes 1, log2 chroma subsampling (0, 0), (1, 0) or (1, 1): yuv444p, yuv422p,
 * yuv420p, FFmpeg's default for a movie).  The planes are decoded exactly, by the RFC: Y, then Cb, then Cr, 8-bit samples, the
 * run index restarting at each plane, the chroma rectangle of a slice at (x0 >> hs, y0 >> vs) with ceil(sw / 2^hs) x
 * ceil(sh / 2^vs) samples.  Only slice grids whose every origin is a multiple of the subsampling are read (then the chroma
 * rectangles tile the chroma plane); others are refused when the stream is opened.  The frames handed out are RGB / BGR as for
 * any other file, converted BY DECREE, not by observation of swscale or cv2 (neither exists here): for pixel (x, y),
 *     Y = Yp[y][x], U = Cb[y >> vs][x >> hs], V = Cr[y >> vs][x >> hs]      (chroma replicated, not interpolated)
 *     c = Y - 16, d = U - 128, e = V - 128                                  (32-bit signed, arithmetic right shift)
 *     R = clip8((298 c + 409 e + 128) >> 8)
 *     G = clip8((298 c - 100 d - 208 e + 128) >> 8)
 *     B = clip8((298 c + 516 d + 128) >> 8)
 * which is BT.601 limited range, swscale's default for a file that signals nothing.  A Matroska Colour element is ignored.
 * Refused with a message: YCbCr with alpha, more than 8 bits, chroma_planes 0 (grey), other subsampling shifts, misaligned grids.
 *
 * What it replaces in the reference:
 *   reader  cv2.VideoCapture(depth_video / color_video) + .read()             stereo_rerender.py:326-341, 489-509
 *           (the toolbox's own *_depth.mkv files; a colour video only if it is FFV1-in-Matroska too: H.264 etc. are not decoded)
 *   writer  cv2.VideoWriter(path, fourcc('F','F','V','1'), fps, (w, h)) + .write()   stereo_rerender.py:426-444, 941;
 *                                                                              depth_frames_helper.py:125-161
 * INTEROPERABILITY UNPINNED: no FFmpeg exists here to read these files or to produce files for the reader.  The encoder is
 * checked by an independent decoder restated from the RFC's pseudo-code (test infrastructure: ffv1_ref.py next to the C oracle), the container by structural
 * tests (EBML sizes, CRCs); tests/golden/gen_ffv1_golden.py produces cross-check vectors on a machine that has ffmpeg.
 * The encoder has a device twin in libmdvt_hip.so, mdvt_encode_video_frames of include/mdvt.h: it codes batches of device frames into
 * the same packets byte for byte, for mdvt_video_write_packet.  The decoder has one too, mdvt_decode_video_frames of
 * include/mdvt_ffv1_decode.h: packets of the stream class this writer makes, in device memory, into the frames mdvt_video_read gives.
 */
#ifndef MDVT_VIDEO_H
#define MDVT_VIDEO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDVT_VIDEO_ABI 1

typedef struct mdvt_video_reader mdvt_video_reader;
typedef struct mdvt_video_writer mdvt_video_writer;

typedef struct mdvt_video_info {
    int32_t width, height;
    int64_t frames;              /* video frames indexed in the file                                   */
    double fps;                  /* from the track's DefaultDuration (or the Info duration / frames)   */
    int32_t ffv1_version;        /* 0, 1 or 3                                                          */
    int32_t ffv1_micro_version;
    int32_t coder_type;          /* 0 Golomb-Rice, 1 range coder default table, 2 range coder custom   */
    int32_t slices;              /* per frame (1 for versions 0 / 1)                                   */
    int32_t alpha;               /* the stream carries a fourth plane (ignored on output)              */
    int32_t intra;               /* every frame is a key frame                                         */
    int32_t ec;                  /* slices end in a CRC-32 parity                                      */
    int32_t pix_fmt;             /* MDVT_VIDEO_PIX_*: what the stream codes (the frames read are RGB / BGR whatever it is) */
} mdvt_video_info;

/* mdvt_video_info.pix_fmt: colorspace_type 1 (the JPEG 2000 RCT over R, G, B), or colorspace_type 0 (YCbCr) with the chroma
 * planes subsampled by log2 (0, 0), (1, 0), (1, 1). */
enum { MDVT_VIDEO_PIX_RGB = 0, MDVT_VIDEO_PIX_YUV444P = 1, MDVT_VIDEO_PIX_YUV422P = 2, MDVT_VIDEO_PIX_YUV420P = 3 };

/* Pixel order of the caller's interleaved 8-bit buffers. */
enum { MDVT_VIDEO_RGB = 0, MDVT_VIDEO_BGR = 1 };   /* BGR = what cv2 hands the reference (sr:489-509 convert it) */

/* 0 on success; a negative code otherwise, with a message in mdvt_video_last_error() (thread local). */
const char* mdvt_video_last_error(void);
int mdvt_video_abi(void);

/* Opens a Matroska file, finds its (first) FFV1 video track, parses the configuration and indexes the frames. */
int mdvt_video_open(const char* path, mdvt_video_reader** out, mdvt_video_info* info);
/* Decodes the NEXT frame (streams with inter-frame context state must be read in order) into dst: height rows of 3*width
 * bytes, `pitch` bytes apart.  threads <= 0: one per slice, capped at the host's cores.  Returns 1 at the end of the video. */
int mdvt_video_read(mdvt_video_reader* r, uint8_t* dst, size_t pitch, int order, int threads);
/* Restarts at frame 0 (a key frame). */
int mdvt_video_rewind(mdvt_video_reader* r);
/* Makes `frame` the next one mdvt_video_read returns.  Free for an intra-only stream; otherwise the frames from the last key
 * frame at or before it are decoded and dropped (a key frame is a packet whose first range-coded bit is 1).  frame == frames:
 * the end. */
int mdvt_video_seek(mdvt_video_reader* r, int64_t frame, int threads);
/* The next frame's FFV1 packet as stored, without decoding it (remuxing); advances like mdvt_video_read.  1 at the end. */
int mdvt_video_next_packet(mdvt_video_reader* r, uint8_t* packet, size_t packet_cap, size_t* packet_size);
/* The stream's configuration record (empty for versions 0 / 1). */
int mdvt_video_config_record(mdvt_video_reader* r, uint8_t* config, size_t config_cap, size_t* config_size);
void mdvt_video_close(mdvt_video_reader* r);

/* Creates path and writes the headers.  FFV1 version 3, range coder (default table), intra-only, RGB colour space, 8 bits,
 * slices_h x slices_v slices (each >= 1, product <= 1024; 0, 0 = 4 x 4), CRC-32 parities.  fps as a rational. */
int mdvt_video_create(const char* path, int width, int height, int fps_num, int fps_den, int slices_h, int slices_v,
                      mdvt_video_writer** out);
/* Encodes one frame (threads as above) and appends it. */
int mdvt_video_write(mdvt_video_writer* w, const uint8_t* src, size_t pitch, int order, int threads);
/* Appends a frame already encoded by mdvt_ffv1_encode_frame with this writer's width, height and slice counts (frames encoded in
 * parallel by the caller, or taken from another file of the same configuration with mdvt_video_next_packet). */
int mdvt_video_write_packet(mdvt_video_writer* w, const uint8_t* packet, size_t packet_size);
/* Writes the cues, patches the duration and the segment size, closes the file; *frames = frames written.  The writer is freed. */
int mdvt_video_finish(mdvt_video_writer* w, int64_t* frames);

/* The codec alone (tests, the independent decoder's counterpart): one frame <-> one FFV1 packet + the configuration record. */
int mdvt_ffv1_encode_frame(int width, int height, int slices_h, int slices_v, const uint8_t* src, size_t pitch, int order,
                           int threads, uint8_t* packet, size_t packet_cap, size_t* packet_size,
                           uint8_t* config, size_t config_cap, size_t* config_size);
/* One packet of a stream with this configuration record (version 3) -> width x 3 bytes of each of height rows of dst: what
 * mdvt_video_read gives for a key frame (an inter frame has no predecessor here and is refused). */
int mdvt_ffv1_decode_frame(int width, int height, const uint8_t* config, size_t config_size, const uint8_t* packet, size_t packet_size,
                           uint8_t* dst, size_t pitch, int order, int threads);

#ifdef __cplusplus
}
#endif
#endif
