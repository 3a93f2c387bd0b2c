/*
 * mdvt_video_stream.h -- the inter-coded stream class on the host, next to include/mdvt_video.h (libmdvt_video.so): a writer for
 * it, and a decoder that keeps its context state from packet to packet without a file around it.
 *
 * mdvt_video_create writes what this project writes by default: range coder, every frame a key frame.  FFmpeg and OpenCV write
 * another class by default -- version 3, coder_type 0 (Golomb-Rice with run mode), intra = 0, a key frame every 12 frames --, and
 * the device reads it with mdvt_decode_video_stream (include/mdvt_ffv1_stream_decode.h).  The writer here makes files of that
 * class at full size in reasonable time (tests, measurements); its packets and configuration record are byte for byte those of
 * the independent restatement ffv1_ref.py's StreamEncoder(Params(coder=0, intra=0, nh, nv), W, H, gop).  Whether FFmpeg reads them is as unpinned as
 * for mdvt_video.h's writer.
 */
#ifndef MDVT_VIDEO_STREAM_H
#define MDVT_VIDEO_STREAM_H

#include <stddef.h>
#include <stdint.h>

#include "mdvt_video.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mdvt_ffv1_stream_decoder mdvt_ffv1_stream_decoder;

/* mdvt_video_create for the stream class: FFV1 version 3.4, coder_type 0 (the only value taken here), intra = 0, frame k a key
 * frame when k % gop == 0 (gop >= 1), RGB, 8 bits, CRC-32 parities.  The writer is used and finished like any other
 * (mdvt_video_write, mdvt_video_finish); a packet handed to mdvt_video_write_packet must continue the stream. */
int mdvt_video_create_stream(const char* path, int width, int height, int fps_num, int fps_den, int slices_h, int slices_v, int coder_type,
                             int gop, mdvt_video_writer** out);

/* Makes `frame` the next one mdvt_video_next_packet returns, without decoding anything on the way (mdvt_video_seek decodes an
 * inter-coded stream forward from its last key frame).  A mdvt_video_read that follows must find a key frame there. */
int mdvt_video_seek_packet(mdvt_video_reader* r, int64_t frame);

/* 1 when `frame`'s packet is a key frame (its first range-coded bit, read from the packet's first two bytes in the file), 0 when
 * not; the reader's position stays where it is. */
int mdvt_video_packet_is_key(mdvt_video_reader* r, int64_t frame);

/* A decoder for consecutive packets of one stream with this configuration record (version 3): what mdvt_video_read does with the
 * packets of a file, YCbCr streams included (converted to RGB / BGR as include/mdvt_video.h states; a slice grid off the chroma
 * grid of this frame size is refused here).  The first packet must be a key frame.  It is the arbiter of the device's
 * mdvt_decode_video_stream. */
int mdvt_ffv1_stream_decoder_create(int width, int height, const uint8_t* config, size_t config_size, mdvt_ffv1_stream_decoder** out);
/* Decodes the next packet into width x 3 bytes of each of height rows of dst (threads as for mdvt_video_read). */
int mdvt_ffv1_stream_decoder_decode(mdvt_ffv1_stream_decoder* d, const uint8_t* packet, size_t packet_size, uint8_t* dst, size_t pitch,
                                    int order, int threads);
void mdvt_ffv1_stream_decoder_destroy(mdvt_ffv1_stream_decoder* d);

#ifdef __cplusplus
}
#endif
#endif
