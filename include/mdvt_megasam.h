/* mdvt_megasam.h -- the non-model work of the reference's MegaSAM camera-tracking step (sam_track_video.py, stv:) on the device: the
 * four entry points of libmdvt_hip.so around the DROID tracker, declared outside include/mdvt.h like the MVSAnywhere step's.
 *
 * sam_track_video.py hands every frame of a colour video, a depth video and an optional mask video to the tracker at about 384 x 512
 * pixels: the colour through cv2.resize(INTER_AREA), the decoded depth through torch's nearest-exact resize, the inverted grey mask
 * through torch's bilinear resize, each cropped to a multiple of 8.  It writes the tracker's depth as a depth video and its motion
 * probability as a grey video (depth_frames_helper.save_grayscale_video, dfh:181-232).  Here are those steps: the three ways in
 * (mdvt_area_model_frames, mdvt_tracker_depth, mdvt_tracker_mask) and the way out (mdvt_tracker_outputs), so that a frame stays on
 * the device from the decoder to the writer.
 *
 * All calls only enqueue on `stream` (a hipStream_t; NULL = the default stream): no read-back, no synchronisation but the one the
 * area tables' block may need when it grows.  Pitches and strides are in bytes and 64-bit.  The results do not depend on the launch
 * geometry; there are no atomics.  The kernels are compiled with -ffp-contract=off and IEEE division: every `*`, `+`, `-` and `/`
 * below is one float32 operation, rounded (fl) before the next.  `bgr` 0: pixels are R, G, B; 1: B, G, R.
 *
 * THE NEAREST-EXACT MAP of the second and the fourth call, torch's CPU F.interpolate(mode="nearest-exact") from n_in to n_out values:
 *     nex(x, n_in, n_out) = min(int(floorf(fl(fl(float(x) + 0.5f) * fl(float(n_in) / float(n_out))))), n_in - 1)
 */
#ifndef MDVT_MEGASAM_H
#define MDVT_MEGASAM_H

#include <stddef.h>
#include <stdint.h>

#include "mdvt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Packed video frames to the tracker's planar uint8 image through cv2.resize(INTER_AREA) and a crop (stv:124, 143-148: BGR -> RGB,
 * cv2.resize(rgb, (mid_w, mid_h), interpolation=cv2.INTER_AREA), image[:out_h, :out_w], permute(2, 0, 1)).
 *
 * Input: n_frames frames of in_h rows of in_w pixels of 3 bytes at d_frames + k * frames_stride + row * frames_pitch.  Output: the
 * uint8 tensor [n_frames, 3, out_h, out_w], planes in R, G, B order whatever the input's order: value (k, c, y, x) at
 * d_out + k * out_stride + c * out_plane_stride + y * out_pitch + x.  out_w <= mid_w and out_h <= mid_h: the top-left corner of the
 * resized image; nothing outside it is computed.
 *
 * RESTATED, NOT OBSERVED: OpenCV is not available where this library is built.  The arithmetic is OpenCV's general area path
 * (computeResizeAreaTab, ResizeArea_Invoker).  For one axis with ssize source and dsize destination samples, scale = ssize / dsize in
 * double, and for each d in ascending order
 *     f1 = d * scale, f2 = f1 + scale, cell = min(scale, ssize - f1)
 *     s1 = ceil(f1), s2 = min(floor(f2), ssize - 1), then s1 = min(s1, s2)
 *     taps, in ascending source order:  (s1 - 1, (s1 - f1) / cell)                      where s1 - f1 > 1e-3
 *                                       (s, 1 / cell)                                   for s1 <= s < s2
 *                                       (s2, min(min(f2 - s2, 1), cell) / cell)         where f2 - s2 > 1e-3
 * each weight rounded to float32 once.  With alpha the horizontal and beta the vertical taps of an output pixel, per channel:
 *     buf(row) = sum over the horizontal taps, ascending, from 0:  buf = fl(buf + fl(float(src) * alpha))
 *     first row:  sum = fl(beta * buf);   later rows, ascending:  sum = fl(sum + fl(beta * buf))
 *     out = sum rounded to the nearest integer, a tie to the even one, clamped to [0, 255]
 * The order of summation is the contract: the work is divided over output samples and channels, never over the taps of one output.
 * Equal sizes give the source bytes themselves (one tap of weight 1 per axis): a crop into planes.
 *
 * The tables are built on the host in double (csrc/mdvt_area_table.h), kept with the context by size pair and uploaded on the
 * call's stream when the pairs on the device are others.  A workgroup takes one output row of a tile of output columns and stages
 * the source rows of that output row, over the tile's source columns, in LDS: with 16-byte loads where d_frames, frames_pitch and
 * (more than one frame) frames_stride are multiples of 16 and a row holds 16 bytes (mdvt_megasam_vector_path), byte by byte
 * otherwise.  Both ways give the same bits.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL ctx, d_frames or d_out; any size or n_frames < 1; out_w > mid_w or
 * out_h > mid_h; bgr not 0 or 1; frames_pitch below 3 * in_w, out_pitch below out_w, out_plane_stride below out_h * out_pitch; with
 * more than one frame frames_stride below in_h * frames_pitch or out_stride below 3 * out_plane_stride.
 * MDVT_ERR_UNSUPPORTED, likewise, with a text that names the reason: mid_w > in_w or mid_h > in_h (area enlargement is another
 * algorithm); in_w / mid_w and in_h / mid_h both integers and not both 1 (OpenCV takes its integer-factor path there, with other
 * rounding, unobserved); a size beyond 16384; source rows of one output row that do not fit a workgroup's LDS even one column wide.
 *
 * Footprint: the first out_w bytes of each row of each plane; nothing else.  Workspace: the two tables (8 + 4 * taps bytes per
 * output sample of an axis).  The result depends on no byte beyond the first 3 * in_w of each input row. */
int mdvt_area_model_frames(mdvt_ctx* ctx, int in_w, int in_h, int n_frames,
                           const uint8_t* d_frames, size_t frames_pitch, size_t frames_stride, int bgr,
                           int mid_w, int mid_h, int out_w, int out_h,
                           uint8_t* d_out, size_t out_pitch, size_t out_plane_stride, size_t out_stride,
                           void* stream);

/* 1 where mdvt_area_model_frames reads such frames with 16-byte loads, 0 where it reads them byte by byte (the image is the same):
 * d_frames, frames_pitch and the stride of more than one frame are multiples of 16, and a row has at least 16 bytes (in_w >= 6).
 * A pure function of its arguments: touches no device. */
int mdvt_megasam_vector_path(int in_w, int n_frames, const uint8_t* d_frames, size_t frames_pitch, size_t frames_stride);

/* Depth-coded frames to the tracker's float32 depth through torch's nearest-exact resize and a crop (stv:125-131, 150-154).
 *
 * Input: n_frames depth-coded frames as mdvt_area_model_frames' frames.  The code of a pixel is u = R << 24 | B << 16: the GREEN byte is
 * NOT read (stv:129-130), unlike in the convergence decode.  Output: the float32 tensor [n_frames, out_h, out_w], value (k, y, x) at
 * d_out + k * out_stride + y * out_pitch + 4 * x:
 *     out = fl(float(u) / float32(255^4 / max_depth))       at source pixel (nex(y, in_h, mid_h), nex(x, in_w, mid_w))
 * ONE correctly rounded float32 division (stv:131: a float32 array by a Python float); 255^4 / max_depth is taken in double first.
 * The decode is part of the gather: only out_h * out_w pixels are decoded.  A thread takes four neighbouring pixels of an output row;
 * four values are one 16-byte store where d_out, out_pitch and out_stride are multiples of 16.  Both ways give the same bits.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL ctx, d_frames or d_out; any size or n_frames < 1; out_w > mid_w or
 * out_h > mid_h; bgr not 0 or 1; max_depth not > 0; frames_pitch below 3 * in_w, out_pitch below 4 * out_w; a stride below rows * pitch
 * with more than one frame; d_out, out_pitch or (more than one frame) out_stride not a multiple of 4.  MDVT_ERR_UNSUPPORTED, likewise:
 * in_w * in_h or out_w * out_h >= 2^31.
 *
 * Footprint: the first 4 * out_w bytes of each row of each plane; nothing else.  No workspace. */
int mdvt_tracker_depth(mdvt_ctx* ctx, int in_w, int in_h, int n_frames,
                       const uint8_t* d_frames, size_t frames_pitch, size_t frames_stride, int bgr, double max_depth,
                       int mid_w, int mid_h, int out_w, int out_h,
                       float* d_out, size_t out_pitch, size_t out_stride,
                       void* stream);

/* Mask frames to the tracker's float32 mask through torch's bilinear resize and a crop (stv:156-165).
 *
 * Input: n_frames mask frames as mdvt_area_model_frames' frames.  Per source pixel, OpenCV's 8-bit COLOR_BGR2GRAY in this project's
 * integers, inverted, as a float:
 *     g = (4899 R + 9617 G + 1868 B + 8192) >> 14,    v = fl(float(255 - g) / 255.0f)
 * then F.interpolate(size=(mid_h, mid_w), mode="bilinear") (align_corners=False, no antialias) in the unfused float32 formula of
 * include/mdvt_mvsa.h (its decree and its bound; the same device code, csrc/mdvt_torch_resize.h), the form chosen by
 * mid_w + mid_h <= 128 as there; cropped to out_h x out_w.  Output as mdvt_tracker_depth's.
 *
 * Refusals, footprint and stores as mdvt_tracker_depth's (without max_depth). */
int mdvt_tracker_mask(mdvt_ctx* ctx, int in_w, int in_h, int n_frames,
                      const uint8_t* d_frames, size_t frames_pitch, size_t frames_stride, int bgr,
                      int mid_w, int mid_h, int out_w, int out_h,
                      float* d_out, size_t out_pitch, size_t out_stride,
                      void* stream);

#define MDVT_TRACKER_DEPTH_VIDEO 0
#define MDVT_TRACKER_GREY_VIDEO 1

/* The tracker's float32 planes to the packed frames of a video (stv:222-234).
 *
 * Input: n_frames float32 planes of in_h rows of in_w values at d_planes + k * planes_stride + row * planes_pitch.  Output: n_frames
 * frames of out_h rows of out_w pixels of 3 bytes at d_frames + k * frames_stride + row * frames_pitch, in the order the writer and the
 * device FFV1 encoder take (bgr).
 *
 * mode MDVT_TRACKER_DEPTH_VIDEO (x_megasam.mkv; stv:223-226, 233): the value at (nex(y, in_h, out_h), nex(x, in_w, out_w)), then
 * depth_frames_helper.save_depth_video at equal size: c = clip(v, 0, max_value), NumPy's (a NaN stays, -0 stays), and
 * mdvt_encode_depth's 16-bit code of c for max_depth = max_value (a NaN gives code 0), the device code and the packed stores of
 * mdvt_depth_video_codes (csrc/mdvt_depth_code.h).
 *
 * mode MDVT_TRACKER_GREY_VIDEO (x_megasam_motion.mkv; dfh:211-230, called with max_depth_arg = 1.0): cv2.resize(INTER_LINEAR) on float32
 * as include/mdvt_metric_align.h restates it (skipped at equal size), then with m = float32(max_value)
 *     g = fl(fl(clip(v, 0, m) / m) * 255.0f),    byte = uint8(trunc(g)),    the pixel is three such bytes
 * DECREE: a NaN gives byte 0 (NumPy's cast of a NaN to uint8 is not defined).  An exact 2 x reduction on both axes is
 * MDVT_ERR_UNSUPPORTED: cv2 takes its area mean there, as elsewhere in this library.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL ctx, d_planes or d_frames; mode not 0 or 1; any size or
 * n_frames < 1; bgr not 0 or 1; max_value not > 0; planes_pitch below 4 * in_w, frames_pitch below 3 * out_w; a stride below
 * rows * pitch with more than one frame; d_planes, planes_pitch or (more than one frame) planes_stride not a multiple of 4.
 * MDVT_ERR_UNSUPPORTED, likewise: out_w * out_h >= 2^31; mode 1 with in_w = 2 * out_w and in_h = 2 * out_h.
 *
 * Footprint: the first 3 * out_w bytes of each row of each frame; nothing else.  No workspace. */
int mdvt_tracker_outputs(mdvt_ctx* ctx, int mode, int in_w, int in_h, int n_frames,
                         const float* d_planes, size_t planes_pitch, size_t planes_stride, double max_value,
                         int out_w, int out_h,
                         uint8_t* d_frames, size_t frames_pitch, size_t frames_stride, int bgr,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif
