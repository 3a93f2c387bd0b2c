/* mdvt_infill_adapter.h -- the frames around an in-painting model on the device: the four entry points of libmdvt_hip.so behind the
 * reference's stereo_crafter_infill.py:101-188 ("scr") and infill_common.py:52-130 ("ic"), declared outside include/mdvt.h like the FFV1
 * decoder's, the convergence depths' and the metric alignment's.
 *
 * The reference's default infill engine is a diffusion in-painter wrapped in per-frame host code: split the side-by-side frame into
 * its eyes, mirror the left one, resize image and mask to the model's size, match the model's colours to its input frame by frame,
 * resize back, paste under the mask and blend along the holes' lower side.  The model is the caller's; everything around it is here.
 *
 * All four calls only enqueue on `stream` (a hipStream_t; NULL = the default stream), take 64-bit pitches and strides (bytes; frame k of
 * an array lies at base + k * stride, row y of a frame at + y * pitch) and refuse a bad layout with MDVT_ERR_INVALID_ARG before anything is
 * launched or written: a NULL ctx or buffer, a size or frame count below 1, a pitch below a row, a stride below rows * pitch with more
 * than one frame, a uint32, uint64 or double array that is not aligned to its element.  Images are u8 RGB, three bytes per pixel.
 *
 * THE U8 RESIZE, used by both adapter calls: cv2.resize(src, (out_w, out_h)) (INTER_LINEAR) on uint8 as OpenCV's plain C++ path
 * states it, RESTATED, not observed (there is no OpenCV where the library is built).  Per output column dx:
 *     f = float32((dx + 0.5) * (in_w / out_w) - 0.5), evaluated in double and rounded once;  sx = floor(f);  f -= sx;
 *     sx < 0 -> sx = 0, f = 0;   sx >= in_w - 1 -> sx = in_w - 1, f = 0;
 *     a0 = rint(fl(1 - f) * 2048), a1 = rint(f * 2048) (half to even);   h = S[sx] * a0 + S[min(sx + 1, in_w - 1)] * a1  in int32.
 * Rows: the same f, sy, b0, b1, but f is NOT zeroed at the borders; the two source rows are clamp(sy, 0, in_h - 1) and
 * clamp(sy + 1, 0, in_h - 1).  Output byte = min((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2, 255).  Equal sizes
 * are a copy; in_w = 2 out_w and in_h = 2 out_h is cv2's area path, (a + b + c + d + 2) >> 2 of the 2 x 2 block.  Channels are independent.
 */
#ifndef MDVT_INFILL_ADAPTER_H
#define MDVT_INFILL_ADAPTER_H

#include <stddef.h>
#include <stdint.h>

#include "mdvt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* scr:101-126.  n_frames side-by-side colour frames and infill-mask frames of eye_h rows of 2 * eye_w pixels; `eye` 0 = the left
 * half read mirrored (np.fliplr), 1 = the right half as it is.  Per frame:
 *     d_image       the eye resized to model_w x model_h (the u8 resize above)
 *     d_model_mask  model_h rows of model_w bytes: the plane (mask pixel != (0,0,0) ? 255 : 0) resized likewise, then > 0 -> 255, else 0
 *     d_hole_counts one uint32 in DEVICE memory: the 255s written to that frame's mask (0 = the frame has no hole: scr:134, 141)
 *
 * MDVT_ERR_INVALID_ARG also: eye not 0 or 1; color_pitch or mask_pitch below 6 * eye_w, image_pitch below 3 * model_w,
 * model_mask_pitch below model_w.  MDVT_ERR_UNSUPPORTED, likewise before anything is written: model_h > 65535.
 *
 * Footprint: the first 3 * model_w bytes of each row of each image, the first model_w bytes of each row of each mask, the n_frames
 * counts (every one is written: they may arrive poisoned); nothing else.  No workspace.  The result depends on no byte outside the
 * eye's 3 * eye_w bytes of each input row. */
int mdvt_adapter_prepare_eye(mdvt_ctx* ctx, int eye_w, int eye_h, int n_frames, int eye,
                             const uint8_t* d_color, size_t color_pitch, size_t color_stride,
                             const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride,
                             int model_w, int model_h,
                             uint8_t* d_image, size_t image_pitch, size_t image_stride,
                             uint8_t* d_model_mask, size_t model_mask_pitch, size_t model_mask_stride,
                             uint32_t* d_hole_counts, void* stream);

/* The integer moments behind transfer_lhm_video_refmask (ic:98-103, 110-118).  Per frame of n_frames frames of height rows of width
 * pixels, over the pixels that count -- all of them where d_mask is NULL, else those whose mask byte (one byte per pixel) is 0 --
 * ten uint64 in DEVICE memory at d_out + 10 * k:
 *     count,  sum r, sum g, sum b,  sum rr, sum rg, sum rb, sum gg, sum gb, sum bb.
 * Exact integers: the result does not depend on the launch geometry.  (A lane sums at most 65536 pixels in 32 bits -- 65536 * 255^2
 * < 2^32 -- before it widens; workgroups join by 64-bit integer atomics.  No floating-point atomics.)
 *
 * THE HOST ALGEBRA that turns two sets of moments into the 15 doubles of mdvt_lhm_apply is float64 and exactly this (NumPy), so that
 * two builds agree:  mu = S1 / n;  cov = float64(n * S2 - S1 S1^T, formed exactly in integers) / (float(n) * max(n - 1, 1));
 * cov = 0.5 * (cov + cov^T);  diagonal += 1e-5;  eigh;  invsqrt_x = (V * (1 / sqrt(clip(w, 1e-5, None)))) @ V^T of the video frame's;
 * sqrt_r = (V * sqrt(clip(w, 0, None))) @ V^T of the reference's;  A = sqrt_r @ invsqrt_x.  A reference with fewer than 3 counted
 * pixels uses its all-pixel moments (ic:113-114).
 *
 * THE FLOAT64 CHOICE.  The reference defaults to single_precision=True, whose X.mean(axis=0) is a sequential float32 sum of H * W
 * terms that no parallel sum reproduces; at 2 x 768 x 1024 x 3 values it differs from its own single_precision=False in 3.2 % of the
 * values, each by 1.  The device follows single_precision=False, which the float32 path approximates, from exact moments.
 *
 * Footprint: exactly the 10 * n_frames uint64 of d_out (every one is written); nothing else.  No workspace.  The result depends on no
 * byte beyond the first 3 * width (mask: width) of each row. */
int mdvt_lhm_moments(mdvt_ctx* ctx, int width, int height, int n_frames,
                     const uint8_t* d_rgb, size_t pitch, size_t stride,
                     const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride,
                     uint64_t* d_out, void* stream);

/* ic:102, 126-128.  d_params: 15 doubles per frame in DEVICE memory at d_params + 15 * k: A row-major, mu_x, mu_r.  Per pixel X:
 *     x_d = double(X_d) - mu_x[d];   y_c = ((x_0 * A[c][0] + x_1 * A[c][1]) + x_2 * A[c][2]) + mu_r[c]
 * every product and sum rounded (no fused multiply-add); output byte = clip(rint(y_c), 0, 255), rint half to even (np.round).
 *
 * MDVT_ERR_UNSUPPORTED, before anything is written: height > 65535.
 * Footprint: the first 3 * width bytes of each row of each output frame; nothing else.  No workspace. */
int mdvt_lhm_apply(mdvt_ctx* ctx, int width, int height, int n_frames,
                   const uint8_t* d_rgb, size_t pitch, size_t stride,
                   const double* d_params,
                   uint8_t* d_out, size_t out_pitch, size_t out_stride, void* stream);

/* scr:151-188.  n_frames model frames of one eye (model_w x model_h; the left eye's are read mirrored: they show the mirrored eye) and
 * the side-by-side colour and infill-mask frames they belong to -> that eye's half (eye_w pixels from column eye * eye_w) of two
 * side-by-side outputs.  With M = the model frame resized to eye_w x eye_h (the u8 resize above), C and K the eye's half of the colour
 * and mask frame as stored (not mirrored):
 *     pasted  (scr:164-169; feeds the chunk overlap) = K != (0,0,0) ? M : C
 *     alpha   = mark_lower_side(K, 30 steps) as mdvt_mark_lower_side, the marks grown by six 4-neighbour dilations (scipy's
 *               binary_dilation(iterations=6): the image border is background), then cv2.GaussianBlur(., (15, 15), 0) of that 0 / 1
 *               image in float32, BORDER_REFLECT_101
 *     blended (scr:183-188; goes to the file) = trunc(clip(fl(fl(alpha * M) + fl(fl(1 - alpha) * pasted)), 0, 255)) in float32
 * The Gaussian: weights exp(-(i - 7)^2 / (2 * 2.6^2)), i = 0..14, normalised in double, rounded once to float32; a horizontal pass,
 * then a vertical one, each a 15-term sum from the first tap on with every product and sum rounded.  These bits are RESTATED, not
 * observed: OpenCV's row filter may fuse multiply and add on the CPU the reference ran on, so a difference of 1 from cv2 is possible
 * where the blend lands on an integer.  No byte parity with cv2 is claimed for the Gaussian or the resize.
 *
 * MDVT_ERR_INVALID_ARG also: eye not 0 or 1; color_pitch, mask_pitch, pasted_pitch or blended_pitch below 6 * eye_w, model_pitch below
 * 3 * model_w.  MDVT_ERR_UNSUPPORTED, before anything is written: eye_w or eye_h below 8 (the reflected 15-tap window); eye_h >
 * 65535; the marches' limits mask_pitch >= 2^24 or mask_pitch * eye_h >= 2^32.
 *
 * Workspace: a scratch block of the context, about 24 + 8 bytes per pixel of ONE eye (the frames run one after the other), under
 * the context's growth rule: the first call allocates it, and a later call with a larger eye waits for the device once
 * (hipDeviceSynchronize) before the smaller block is replaced; a call that needs no more than an earlier one never waits.
 *
 * Footprint: bytes [3 * eye * eye_w, 3 * (eye + 1) * eye_w) of each row of each pasted and blended frame (every one is written);
 * nothing else of the caller's.  The outputs may not overlap the inputs. */
int mdvt_adapter_composite_eye(mdvt_ctx* ctx, int eye_w, int eye_h, int n_frames, int eye,
                               const uint8_t* d_model, int model_w, int model_h, size_t model_pitch, size_t model_stride,
                               const uint8_t* d_color, size_t color_pitch, size_t color_stride,
                               const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride,
                               uint8_t* d_pasted, size_t pasted_pitch, size_t pasted_stride,
                               uint8_t* d_blended, size_t blended_pitch, size_t blended_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif
