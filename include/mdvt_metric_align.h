/* mdvt_metric_align.h -- relative inverse depth to a metric depth video on the device: the two entry points of libmdvt_hip.so behind
 * the reference's video_metric_convert.py:17-41, 101-149, depthcrafter_video.py:19-43, 200-252 and geometrycrafter_video.py:244,
 * declared outside include/mdvt.h like the FFV1 decoder's and the convergence depths'.
 *
 * The video-consistent depth models (Video-Depth-Anything, DepthCrafter, GeometryCrafter) give relative inverse depth.  The
 * reference fits `1 / metric = scale * rel + shift` over the first frames against a metric reference (compute_scale_and_shift_full),
 * inverts every pixel, resizes to the video's size and writes the 16-bit RGB depth code (depth_frames_helper.save_depth_video).  The
 * fit feeds every depth of the clip, so the device gives the reference's float32 numbers bit for bit.
 */
#ifndef MDVT_METRIC_ALIGN_H
#define MDVT_METRIC_ALIGN_H

#include <stddef.h>
#include <stdint.h>

#include "mdvt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* compute_scale_and_shift_full(prediction, target, mask) over n_frames planes of `height` rows of `width` float32 values, plane k
 * of the prediction at d_pred + k * pred_stride + row * pred_pitch (bytes), of the target and of the mask likewise.  The summed
 * arrays are the planes concatenated: n = n_frames * height * width values in frame-major, row-major order.
 *
 *     p = prediction, m = float32(mask byte) (1 where d_mask is NULL: a bool or uint8 mask's astype(float32)),
 *     t = target (target_is_depth 0), or float32(1) / target, one correctly rounded division (target_is_depth 1)
 *     a_00 = sum((m * p) * p)   a_01 = sum(m * p)   a_11 = sum(m)   b_0 = sum((m * p) * t)   b_1 = sum(m * t)
 *     det = a_00 * a_11 - a_01 * a_01
 *     det != 0 (a NaN is):  scale = (a_11 * b_0 - a_01 * b_1) / det,  shift = (-a_01 * b_0 + a_00 * b_1) / det;  else scale = 1, shift = 0
 *
 * All in float32, every product and sum rounded before the next (no fused multiply-add).  Each sum is NumPy's np.sum of the
 * contiguous float32 array: the order include/mdvt_convergence.h states (chunks of 8192 values, the pairwise routine pw, the chunk
 * sums added one after the other from 0), without the final division.  inf and NaN (a depth of 0 gives t = inf) follow IEEE in that
 * order.
 *
 * d_out: 8 floats in DEVICE memory: a_00, a_01, a_11, b_0, b_1, scale, shift, det.
 *
 * The call only enqueues on `stream` (a hipStream_t; NULL = the default stream): no read-back, no synchronisation, no
 * floating-point atomics; the result is independent of the launch geometry.  The chunk sums (5 * 4 B per chunk) live in a scratch
 * block of the context; inputs of more than 1024 chunks run in launch sets of that many, so the block never exceeds 21 KiB, below
 * any mdvt_config.workspace_mib.  The one exception to "no synchronisation": the block follows the context's growth rule, so a
 * context's first fit allocates it, and a later fit of more chunks than any before (up to 1024) waits for the device once
 * (hipDeviceSynchronize) before the smaller block is replaced.  A fit of at most as many chunks as an earlier one never waits.
 *
 * A plane is read with 16-byte loads where its address, pitch and stride are multiples of 16 and width is a multiple of 4 (a
 * mask: 4-byte loads, multiples of 4), or where it has no padding at all (pitch = 4 * width, stride = height * pitch; mask: width)
 * and its address is a multiple of 16 (mask: 4); element by element otherwise.  Both ways give the same bits.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL ctx, d_pred, d_target or d_out; width or height < 1;
 * n_frames < 1; a pitch below 4 * width (mask: width); a stride below height * pitch with more than one frame; target_is_depth
 * not 0 or 1.  MDVT_ERR_UNSUPPORTED, likewise: n_frames * width * height >= 2^31.
 *
 * Footprint: exactly the 8 floats of d_out; nothing else of the caller's.  The result depends on no byte beyond the first
 * 4 * width (mask: width) of each row. */
int mdvt_scale_shift_fit(mdvt_ctx* ctx, int width, int height, int n_frames,
                         const float* d_pred, size_t pred_pitch, size_t pred_stride,
                         const float* d_target, size_t target_pitch, size_t target_stride, int target_is_depth,
                         const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride,
                         float* d_out, void* stream);

/* Metric depth codes of n_frames relative planes x of in_h rows of in_w float32 values at d_rel + k * rel_stride + row * rel_pitch.
 * d_scale_shift: two floats in DEVICE memory, scale then shift (d_out + 5 of mdvt_scale_shift_fit on the same stream: no read-back).
 *
 * Reconstruction, float32, each step rounded (fl):  inv = fl(fl(x * scale) + shift), then
 *     style 0 (video_metric_convert.py:136-142):  d = fl(1 / inv);  d < 0 -> float32(max_depth)
 *     style 1 (depthcrafter_video.py:236-243):    inv == 0 -> float32(1e-4);  d = clip(fl(1 / inv), 0, max_depth);  NaN -> max_depth;
 *                                                 after the resize clip(., 0, max_depth) once more
 * clip is NumPy's: min(max(d, 0), max_depth), a NaN stays.
 *
 * Resize to out_w x out_h (skipped when both sizes are equal): cv2.resize(d, (out_w, out_h), INTER_LINEAR) on float32 as OpenCV's
 * source states it, RESTATED, not observed.  Per output column dx: fx = float32((dx + 0.5) * (in_w / out_w) - 0.5) evaluated in
 * double and rounded once; sx = floor(fx); fx -= sx; sx < 0 -> sx = 0, fx = 0; sx >= in_w - 1 -> sx = in_w - 1, fx = 0; weights
 * a0 = 1 - fx, a1 = fx; sx1 = min(sx + 1, in_w - 1).  Rows likewise (b0, b1).  r = fl(fl(S[sx] * a0) + fl(S[sx1] * a1)) on the two
 * source rows, then fl(fl(r0 * b0) + fl(r1 * b1)).  No fused multiply-add.
 *
 * Code (depth_frames_helper.py:5-11, 48-61, as mdvt_encode_depth): c = clip(d, 0, max_depth) in float32;
 * u = uint32(trunc((255^4 / max_depth) * double(c))); R = G = byte 3 of u, B = byte 2.  A NaN c (style 0 only) has no defined
 * conversion in the reference; the library writes code 0 and leaves the NaN in the depth plane.
 *
 * Outputs: n_frames code images of out_h rows of out_w pixels of 3 bytes (order 0: R, G, B; 1: B, G, R) at d_codes + k * codes_stride
 * + row * codes_pitch and, where d_depth is not NULL, the float32 planes of c at d_depth + k * depth_stride + row * depth_pitch.
 * Only enqueues on `stream`.  All pitches, strides and frame offsets are 64-bit.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL ctx, d_rel, d_scale_shift or d_codes; any of in_w, in_h,
 * out_w, out_h, n_frames < 1; rel_pitch below 4 * in_w, codes_pitch below 3 * out_w, depth_pitch below 4 * out_w; a stride below
 * rows * pitch with more than one frame; style or order not 0 or 1; max_depth not > 0.  MDVT_ERR_UNSUPPORTED, likewise:
 * out_w * out_h >= 2^31.
 *
 * Footprint: the first 3 * out_w bytes of each row of each code image and, where given, the first 4 * out_w bytes of each row of
 * each depth plane; nothing else.  The result depends on no byte beyond the first 4 * in_w of each input row. */
int mdvt_metric_depth_codes(mdvt_ctx* ctx, int in_w, int in_h, int n_frames,
                            const float* d_rel, size_t rel_pitch, size_t rel_stride,
                            const float* d_scale_shift, int style, double max_depth,
                            int out_w, int out_h,
                            uint8_t* d_codes, size_t codes_pitch, size_t codes_stride, int order,
                            float* d_depth, size_t depth_pitch, size_t depth_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif
