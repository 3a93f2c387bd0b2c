/* mdvt_depth_engines.h -- the non-model work of the reference's per-frame depth engines and of its PromptDA upscaler on the device: the
 * three entry points of libmdvt_hip.so behind unik3d_video.py, moge_video.py, depthpro_video.py and upscale_depth_promptda.py, declared
 * outside include/mdvt.h like the depth sink's.
 *
 * Those scripts decode a frame, hand it to a model and send the model's metric depth to a depth video.  mdvt_depth_video_codes
 * (include/mdvt_depth_sink.h) is the way out.  Here are the three steps in front of it that are not the model's: the frames' way into the
 * model (mdvt_model_frames), PromptDA's low-resolution prompt from a coded depth video (mdvt_depth_prompt) and UniK3D's focal estimate
 * from its point map (mdvt_focal_from_points), so that a frame stays on the device from the decoder to the writer.
 *
 * All three calls only enqueue on `stream` (a hipStream_t; NULL = the default stream): no read-back, no synchronisation but the one the
 * focal estimate's scratch block may need when it grows (below).  Pitches and strides are in bytes and 64-bit, as every frame offset
 * is.  The results do not depend on the launch geometry; there are no floating-point atomics.  The kernels are compiled with
 * -ffp-contract=off and IEEE division: every `*`, `+`, `-` and `/` below is one float32 operation, rounded (fl) before the next.
 */
#ifndef MDVT_DEPTH_ENGINES_H
#define MDVT_DEPTH_ENGINES_H

#include <stddef.h>
#include <stdint.h>

#include "mdvt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Packed video frames to a model's planar input tensor.
 *
 * Input: n_frames frames of in_h rows of in_w pixels of 3 bytes (order 0: R, G, B; 1: B, G, R) at d_frames + k * frames_stride
 * + row * frames_pitch.  Output: the tensor [n_frames, 3, out_h, out_w] with its planes in R, G, B order whatever the input's order:
 * value (k, c, y, x) at d_out + k * out_stride + c * out_plane_stride + y * out_pitch + x * (1 or 4).
 *
 *   1. where (out_w, out_h) != (in_w, in_h) the frame is resized first: cv2.resize(frame, (out_w, out_h), INTER_LINEAR) on uint8, THE U8
 *      RESIZE of include/mdvt_infill_adapter.h operation for operation (the same device code), its exact-2x case
 *      (in_w = 2 out_w and in_h = 2 out_h: the rounded mean of the 2 x 2 block) included.  Channels are independent.
 *   2. format 0: the byte v as it is (uint8; unik3d_video.py:166's permute(2, 0, 1)).
 *      format 1: float32 fl(float(v) / 255.0f), ONE correctly rounded division: NumPy's rgb.astype(float32) / 255 (moge_video.py:159-160)
 *      and torch's CPU .float() / 255.0 (upscale_depth_promptda.py:69) on all 256 values.  It is not v * (1 / 255).
 *
 * A thread takes four neighbouring pixels of an output row.  Without a resize they are one 12-byte load where d_frames, frames_pitch
 * and frames_stride are multiples of 4 (neighbouring lanes read neighbouring 12 bytes: a wave's load is one run of 768 bytes);
 * resized, every pixel gathers its source pixels byte by byte.  Four values of a plane are one 4-byte (format 0) or 16-byte (format 1)
 * store where d_out, out_pitch, out_plane_stride and out_stride are multiples of 4 (format 1: 16); element by element otherwise, and
 * for the last one to three pixels of a row.  Both ways give the same bits.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL ctx, d_frames or d_out; any of in_w, in_h, out_w, out_h,
 * n_frames < 1; order or format not 0 or 1; frames_pitch below 3 * in_w, out_pitch below out_w (format 1: 4 * out_w);
 * out_plane_stride below out_h * out_pitch; with more than one frame frames_stride below in_h * frames_pitch or out_stride below
 * 3 * out_plane_stride; format 1: d_out, out_pitch, out_plane_stride or (more than one frame) out_stride not a multiple of 4 (a
 * float32 is stored at its alignment).  MDVT_ERR_UNSUPPORTED, likewise: in_w * in_h or out_w * out_h >= 2^31.
 *
 * Footprint: the first out_w elements of each row of each plane; nothing else.  No workspace.  The result depends on no byte beyond
 * the first 3 * in_w of each input row. */
int mdvt_model_frames(mdvt_ctx* ctx, int in_w, int in_h, int n_frames,
                      const uint8_t* d_frames, size_t frames_pitch, size_t frames_stride, int order,
                      int out_w, int out_h, int format,
                      void* d_out, size_t out_pitch, size_t out_plane_stride, size_t out_stride,
                      void* stream);

/* Coded depth frames to PromptDA's low-resolution prompt (upscale_depth_promptda.py:59-62): decode_rgb_depth_frame, then
 * cv2.resize(INTER_LINEAR) on float32, in one pass.
 *
 * Input: n_frames depth frames of in_h rows of in_w pixels of 3 bytes (order 0: R, G, B; 1: B, G, R) at d_codes + k * codes_stride
 * + row * codes_pitch.  A pixel's depth is mdvt_decode_depth's: fl(float32(R << 24 | B << 16) * float32(max_depth / 255^4)) (dfh:21-23;
 * G is ignored, the factor is computed in double and rounded once).
 *
 * Output: n_frames float32 planes of out_h rows of out_w values at d_prompt + k * prompt_stride + row * prompt_pitch.  Equal sizes
 * give the plain decode.  Otherwise each output value takes the four source taps of cv2.resize(INTER_LINEAR) on float32 exactly as
 * include/mdvt_metric_align.h restates it -- the same tables, r = fl(fl(S[sx] * a0) + fl(S[sx1] * a1)) on the two source rows, then
 * fl(fl(r0 * b0) + fl(r1 * b1)) -- and decodes each tap where it gathers it: a 1920 x 1080 frame to 256 x 192 reads about 0.2 MB,
 * not 6 MB, and no full-size float plane exists.
 *
 * A thread takes four neighbouring output values.  Without a resize their codes are one 12-byte load where d_codes, codes_pitch and
 * codes_stride are multiples of 4; they are one 16-byte store where d_prompt, prompt_pitch and prompt_stride are multiples of 16;
 * element by element otherwise.  Both ways give the same bits.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL ctx, d_codes or d_prompt; any of in_w, in_h, out_w, out_h,
 * n_frames < 1; order not 0 or 1; max_depth not > 0; codes_pitch below 3 * in_w, prompt_pitch below 4 * out_w; a stride below
 * rows * pitch with more than one frame; d_prompt, prompt_pitch or (more than one frame) prompt_stride not a multiple of 4.
 * MDVT_ERR_UNSUPPORTED, likewise: in_w = 2 out_w and in_h = 2 out_h (OpenCV leaves its
 * linear path for its area path there, and what that path rounds cannot be observed where this library is built); in_w * in_h or
 * out_w * out_h >= 2^31.
 *
 * Footprint: the first 4 * out_w bytes of each row of each plane; nothing else.  No workspace.  The result depends on no byte beyond
 * the first 3 * in_w of each input row. */
int mdvt_depth_prompt(mdvt_ctx* ctx, int in_w, int in_h, int n_frames,
                      const uint8_t* d_codes, size_t codes_pitch, size_t codes_stride, int order, double max_depth,
                      int out_w, int out_h,
                      float* d_prompt, size_t prompt_pitch, size_t prompt_stride,
                      void* stream);

/* UniK3D's focal estimate from its point map (estimate_focal_lengths, unik3d_video.py:22-101), per frame.
 *
 * Input: n_frames point maps of height rows of width points (X, Y, Z), float32.  layout 0 is [n, 3, H, W]: coordinate c of point
 * (v, u) of frame k at d_points + k * points_stride + c * points_plane_stride + v * points_pitch + 4 * u.  layout 1 is [n, H, W, 3]:
 * at d_points + k * points_stride + v * points_pitch + 12 * u + 4 * c (points_plane_stride is ignored).
 *
 * Per point (u, v), in float32, each step rounded:
 *     ex = fl(fl(u - width / 2) * fl(Z / X)),   selected where |X| > 1e-6f && |Z| > 1e-6f
 *     ey = fl(fl(v - height / 2) * fl(Z / Y)),  selected where |Y| > 1e-6f && |Z| > 1e-6f
 * The threshold is float32(1e-6); torch's comparison against the double 1e-6 selects the same float32 values.  A NaN selects nothing;
 * an infinity is selected and IEEE decides what it gives.  Z / X is one IEEE division; u - width / 2 is exact (the size limit below).
 *
 * d_focal[2 k] = fx, the float32 mean of the nx selected ex of frame k in row-major order; d_focal[2 k + 1] = fy likewise from the ny
 * selected ey.  A frame that selects nothing gives 0.0f (unik3d_video.py:98-99).  Where d_counts is not NULL, d_counts[2 k] = nx and
 * d_counts[2 k + 1] = ny.
 *
 * DECREE.  The reference sums with torch on CUDA, whose order of summation cannot be observed where this library is built.  The
 * values ex, ey and both selections are torch's bit for bit.  The ORDER of the sum is this project's: NumPy's float32 mean over the
 * compacted sequence, as include/mdvt_convergence.h states it and mdvt_convergence_depths takes it under a mask -- consecutive chunks of
 * 8192 values, each summed by the pairwise routine, the chunk sums added one after the other from 0, the total divided by float32(n).
 * The same device routines do it (csrc/mdvt_pairwise.h).  Two float32 sums of the same n values in any two orders differ by at most
 * 2 (n - 1) 2^-24 sum|e| (to first order), so fx and fy lie within 2 (n - 1) 2^-24 sum|e| / n of torch's means.
 *
 * Workspace (per frame of a launch set about 8 B per point: the selected values of both axes, and a few words per 2048 points)
 * comes from the context's pool and is bounded by mdvt_config.workspace_mib: a large batch runs in launch sets.  The block follows the
 * context's growth rule: a call that needs more than any before waits for the device once before the smaller block is replaced.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL ctx, d_points or d_focal; width, height or n_frames < 1; layout
 * not 0 or 1; points_pitch below 4 * width (layout 1: 12 * width); layout 0: points_plane_stride below height * points_pitch; with
 * more than one frame points_stride below 3 * points_plane_stride (layout 1: height * points_pitch); d_points, points_pitch,
 * points_plane_stride (layout 0) or (more than one frame) points_stride not a multiple of 4; d_focal or d_counts not 4-byte aligned.
 * MDVT_ERR_UNSUPPORTED, likewise: width or height > 2^23, width * height > 2^28.
 *
 * Footprint: exactly 2 * n_frames floats of d_focal and, where given, 2 * n_frames words of d_counts; nothing else of the caller's.
 * The result depends on no byte beyond the first 4 * width (layout 1: 12 * width) of each row. */
int mdvt_focal_from_points(mdvt_ctx* ctx, int width, int height, int n_frames,
                           const float* d_points, int layout, size_t points_pitch, size_t points_plane_stride, size_t points_stride,
                           float* d_focal, uint32_t* d_counts,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
