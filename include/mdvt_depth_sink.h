/* mdvt_depth_sink.h -- metric depth planes to a depth video on the device: the entry point of libmdvt_hip.so behind the reference's
 * depth_frames_helper.save_depth_video (depth_frames_helper.py:125-161), declared outside include/mdvt.h like the metric alignment's.
 *
 * save_depth_video is the sink of every metric-depth script of the reference (video_da3, unidepth_video, unik3d_video, video_mvsa,
 * videoanythingmetric_video, upscale_depth_promptda, moge_video): float32 metric depth at the model's size -> cv2.resize(INTER_LINEAR)
 * to the video's size -> the 16-bit RGB depth code.  mdvt_metric_depth_codes (include/mdvt_metric_align.h) has the same tail behind
 * an inversion; this call takes the depth itself, with the two things the scripts do to it just before: moge_video.py:171 sets NaN to
 * max_depth, video_da3.py:193 multiplies a batch by the scale that aligns it to the batch before.  That scale comes from a fit on the
 * device, so it is taken from device memory: no read-back stands between the fit and the codes.
 */
#ifndef MDVT_DEPTH_SINK_H
#define MDVT_DEPTH_SINK_H

#include <stddef.h>
#include <stdint.h>

#include "mdvt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Depth codes of n_frames metric planes of in_h rows of in_w float32 values at d_depth + k * depth_stride + row * depth_pitch (bytes).
 *
 * Per source value x, in float32, each step rounded (fl), no fused multiply-add:
 *   1. nan_to_max 1 and x != x:  x = float32(max_depth)                                   (moge_video.py:171)
 *   2. d_scale not NULL:  x = fl(x * s), s the one float d_scale points to in DEVICE memory (video_da3.py:193: NumPy multiplies a
 *      float32 array by a Python float in float32).  s may be 0, inf or NaN: IEEE decides.
 *   3. where (in_w, in_h) != (out_w, out_h): cv2.resize(x, (out_w, out_h), INTER_LINEAR) on float32 exactly as
 *      include/mdvt_metric_align.h restates it: the same tables, r = fl(fl(S[sx] * a0) + fl(S[sx1] * a1)) on the two source rows, then
 *      fl(fl(r0 * b0) + fl(r1 * b1)).  A weight of 0 still multiplies: inf * 0 is NaN, as in OpenCV.
 *   4. c = clip(x, 0, max_depth), NumPy's: min(max(x, 0), max_depth), a NaN stays, -0 stays.  The code is mdvt_encode_depth's:
 *      u = uint32(trunc((255^4 / max_depth) * double(c))); R = G = byte 3 of u, B = byte 2.  A NaN c has no defined conversion in the
 *      reference; the library writes code 0 and leaves the NaN in d_plane.
 *
 * Outputs: n_frames code images of out_h rows of out_w pixels of 3 bytes (order 0: R, G, B; 1: B, G, R) at d_codes + k * codes_stride
 * + row * codes_pitch and, where d_plane is not NULL, the float32 planes of c at d_plane + k * plane_stride + row * plane_pitch.
 *
 * The call only enqueues on `stream` (a hipStream_t; NULL = the default stream): no read-back, no synchronisation, no scratch block of
 * the context.  All pitches, strides and frame offsets are 64-bit.  The result is independent of the launch geometry.
 *
 * Four source values are one 16-byte load where no resize happens and d_depth, depth_pitch and depth_stride are multiples of 16; four
 * codes are three 4-byte stores where d_codes, codes_pitch and codes_stride are multiples of 4; four plane values are one 16-byte
 * store where d_plane, plane_pitch and plane_stride are multiples of 16; element by element otherwise.  Both ways give the same bits.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL ctx, d_depth or d_codes; any of in_w, in_h, out_w, out_h,
 * n_frames < 1; depth_pitch below 4 * in_w, codes_pitch below 3 * out_w, plane_pitch below 4 * out_w; a stride below rows * pitch with
 * more than one frame; order or nan_to_max not 0 or 1; max_depth not > 0.  MDVT_ERR_UNSUPPORTED, likewise: out_w * out_h >= 2^31.
 *
 * Footprint: the first 3 * out_w bytes of each row of each code image and, where given, the first 4 * out_w bytes of each row of
 * each plane; nothing else.  The result depends on no byte beyond the first 4 * in_w of each input row. */
int mdvt_depth_video_codes(mdvt_ctx* ctx, int in_w, int in_h, int n_frames,
                           const float* d_depth, size_t depth_pitch, size_t depth_stride,
                           const float* d_scale,
                           int nan_to_max, double max_depth, int out_w, int out_h,
                           uint8_t* d_codes, size_t codes_pitch, size_t codes_stride, int order,
                           float* d_plane, size_t plane_pitch, size_t plane_stride,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
