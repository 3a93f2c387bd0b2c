/* mdvt_mvsa.h -- the non-model work of the reference's MVSAnywhere step (video_mvsa.py) on the device: the three entry points of
 * libmdvt_hip.so around the multi-view model, declared outside include/mdvt.h like the depth engines'.
 *
 * video_mvsa.py turns a frame and its neighbours into float planes with TORCH's bilinear resize (not OpenCV's), hands them with poses
 * and intrinsics to the model, and sends the refined depth through two nearest-neighbour resizes to save_depth_video.  Alongside it
 * computes a masked median ratio between the cost volume's depth and the refined depth, which it leaves unused.  Here are those three
 * steps: the frames' way in (mdvt_bilinear_model_frames), the depth's way out (mdvt_nearest_depth_codes) and the median
 * (mdvt_ratio_median), so that a frame stays on the device from the decoder to the writer.
 *
 * All three calls only enqueue on `stream` (a hipStream_t; NULL = the default stream): no read-back, no synchronisation but the one the
 * median's scratch block may need when it grows (below).  Pitches and strides are in bytes and 64-bit, as every frame offset is.  The
 * results do not depend on the launch geometry; there are no floating-point atomics.  The kernels are compiled with -ffp-contract=off
 * and IEEE division: every `*`, `+`, `-` and `/` below is one float32 operation, rounded (fl) before the next.
 *
 * THE NEAREST MAP of both the second and the third call, torch's CPU F.interpolate(mode="nearest") from n_in to n_out values:
 *     near(x, n_in, n_out) = min(int(floorf(fl(float(x) * fl(float(n_in) / float(n_out))))), n_in - 1)
 */
#ifndef MDVT_MVSA_H
#define MDVT_MVSA_H

#include <stddef.h>
#include <stdint.h>

#include "mdvt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Packed video frames to the model's planar float32 input through torch's bilinear resize (video_mvsa.py:59-63, 165, 200: BGR -> RGB,
 * .float() / 255.0, F.interpolate(size=(out_h, out_w), mode="bilinear", align_corners=False)).
 *
 * Input: n_frames frames of in_h rows of in_w pixels of 3 bytes (order 0: R, G, B; 1: B, G, R) at d_frames + k * frames_stride
 * + row * frames_pitch.  Output: the float32 tensor [n_frames, 3, out_h, out_w], planes in R, G, B order whatever the input's order:
 * value (k, c, y, x) at d_out + k * out_stride + c * out_plane_stride + y * out_pitch + 4 * x.
 *
 * DECREE.  torch's CPU kernel has no single set of bits: they depend on the CPU's vector extension, on the thread count and on
 * whether the build contracts the source index into a fused multiply-add.  The library computes the unfused float32 formula, which
 * is torch's bit for bit where in / out is exactly representable and torch runs its plain (ATEN_CPU_CAPABILITY=default, several
 * threads) kernel, and lies within 2^(ceil(log2 in_w) - 24) + 2^(ceil(log2 in_h) - 24) + 4 * 2^-24 of it otherwise.  Per axis, with n_in
 * source and n_out output values and output index x:
 *     scale = fl(float(n_in) / float(n_out))
 *     src   = max(fl(fl(scale * fl(float(x) + 0.5f)) - 0.5f), 0)
 *     i0    = min(int(src), n_in - 1),   i1 = min(i0 + 1, n_in - 1)
 *     lam   = min(max(fl(src - float(i0)), 0), 1),   w0 = fl(1 - lam),   w1 = lam
 * and with v = fl(float(byte) / 255.0f), ONE correctly rounded division as in mdvt_model_frames' format 1:
 *     t(r)  = fl(fl(wx0 * v[r][x0]) + fl(wx1 * v[r][x1]))
 *     out   = fl(fl(wy0 * t(y0)) + fl(wy1 * t(y1)))
 * That is torch's kernel wherever out_w + out_h > 128, which every size the model takes is.  For smaller outputs torch's CPU dispatch
 * takes another kernel even with the plain capability, and so does the library, so that the library is torch's plain kernel at every
 * size: where out_w + out_h <= 128, with the same indices and weights,
 *     out   = fl(fl(fl(fl(fl(wy0 * wx0) * v[y0][x0]) + fl(fl(wy0 * wx1) * v[y0][x1])) + fl(fl(wy1 * wx0) * v[y1][x0])) + fl(fl(wy1 * wx1) * v[y1][x1]))
 * Equal sizes give v itself in both forms (src = x exactly, lam = 0).  Channels are independent.
 *
 * A thread takes four neighbouring pixels of an output row and gathers their taps byte by byte.  Four values of a plane are one
 * 16-byte store where d_out, out_pitch, out_plane_stride and out_stride are multiples of 16; element by element otherwise, and for
 * the last one to three pixels of a row.  Both ways give the same bits.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL ctx, d_frames or d_out; any of in_w, in_h, out_w, out_h,
 * n_frames < 1; order not 0 or 1; frames_pitch below 3 * in_w, out_pitch below 4 * out_w; out_plane_stride below out_h * out_pitch;
 * with more than one frame frames_stride below in_h * frames_pitch or out_stride below 3 * out_plane_stride; d_out, out_pitch,
 * out_plane_stride or (more than one frame) out_stride not a multiple of 4.  MDVT_ERR_UNSUPPORTED, likewise: in_w * in_h or
 * out_w * out_h >= 2^31.
 *
 * Footprint: the first out_w floats of each row of each plane; nothing else.  No workspace.  The result depends on no byte beyond
 * the first 3 * in_w of each input row. */
int mdvt_bilinear_model_frames(mdvt_ctx* ctx, int in_w, int in_h, int n_frames,
                               const uint8_t* d_frames, size_t frames_pitch, size_t frames_stride, int order,
                               int out_w, int out_h,
                               float* d_out, size_t out_pitch, size_t out_plane_stride, size_t out_stride,
                               void* stream);

/* The refined depth to a depth video's codes through two nearest-neighbour resizes (video_mvsa.py:268, 297-298, then
 * depth_frames_helper.save_depth_video at equal size: clip, then the 16-bit code).
 *
 * Input: n_frames float32 planes of in_h rows of in_w values at d_depth + k * depth_stride + row * depth_pitch.  Output pixel (y, x)
 * takes the source value at the composition of the two nearest maps, first to (mid_w, mid_h), the cost volume's size, then to
 * (out_w, out_h):
 *     mx = near(x, mid_w, out_w),   sx = near(mx, in_w, mid_w);   rows likewise with the heights.
 * Then, as steps 2 and 4 of mdvt_depth_video_codes (include/mdvt_depth_sink.h), the same device code:
 *     d_scale not NULL:  v = fl(v * s), s the one float at d_scale + k * scale_stride in DEVICE memory for frame k (scale_stride may be 0:
 *                        one factor for all frames).  s may be 0, inf or NaN: IEEE decides.
 *     c = clip(v, 0, max_depth), NumPy's: a NaN stays, -0 stays.  The code is mdvt_encode_depth's; a NaN c gives code 0 and stays in d_plane.
 * DECREE: the reference runs the two resizes on CUDA, whose index arithmetic cannot be observed where this library is built; the
 * map is torch's CPU kernel's.  The factor is this project's reading of the reference's commented-out `* s` (video_mvsa.py:297), not
 * the reference's output: without d_scale the call computes what the reference writes.
 *
 * Outputs as mdvt_depth_video_codes': n_frames code images of out_h rows of out_w pixels of 3 bytes (order 0: R, G, B; 1: B, G, R) at
 * d_codes + k * codes_stride + row * codes_pitch and, where d_plane is not NULL, the float32 planes of c at d_plane + k * plane_stride
 * + row * plane_pitch.  Four codes are three 4-byte stores where d_codes, codes_pitch and codes_stride are multiples of 4; four plane
 * values one 16-byte store where d_plane, plane_pitch and plane_stride are multiples of 16; element by element otherwise.  Both ways
 * give the same bits.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL ctx, d_depth or d_codes; any of in_w, in_h, mid_w, mid_h, out_w,
 * out_h, n_frames < 1; order not 0 or 1; max_depth not > 0; depth_pitch below 4 * in_w, codes_pitch below 3 * out_w, plane_pitch below
 * 4 * out_w; a stride below rows * pitch with more than one frame; d_depth, depth_pitch, d_scale, scale_stride, d_plane, plane_pitch or
 * (more than one frame) depth_stride or plane_stride not a multiple of 4.  MDVT_ERR_UNSUPPORTED, likewise: out_w * out_h >= 2^31.
 *
 * Footprint: the first 3 * out_w bytes of each row of each code image and, where given, the first 4 * out_w bytes of each row of
 * each plane; nothing else.  No workspace.  The result depends on no byte beyond the first 4 * in_w of each input row. */
int mdvt_nearest_depth_codes(mdvt_ctx* ctx, int in_w, int in_h, int n_frames,
                             const float* d_depth, size_t depth_pitch, size_t depth_stride,
                             int mid_w, int mid_h,
                             const float* d_scale, size_t scale_stride,
                             double max_depth, int out_w, int out_h,
                             uint8_t* d_codes, size_t codes_pitch, size_t codes_stride, int order,
                             float* d_plane, size_t plane_pitch, size_t plane_stride,
                             void* stream);

/* The masked median ratio between the cost volume's depth and the refined depth (video_mvsa.py:261-293), per frame.
 *
 * Inputs, n_frames of each: the cost volume's depth, float32 planes of cv_h rows of cv_w values at d_cv + k * cv_stride + row *
 * cv_pitch; the refined depth, float32 planes of ref_h x ref_w likewise, sampled at the cost volume's size through the nearest map
 * (ref at (near(y, ref_h, cv_h), near(x, ref_w, cv_w)); video_mvsa.py:268); and, where d_mask is not NULL, uint8 planes of mask_h x
 * mask_w, non-zero = true, sampled likewise (video_mvsa.py:279-280: a bool that goes to float, through nearest, and back to bool is
 * nearest on the bool).  Without a mask every pixel counts as true (video_mvsa.py:276: the `cv > 0` it falls back to is part of
 * `valid` already); mask_w, mask_h, mask_pitch and mask_stride are then ignored.
 *
 *     valid = mask && isfinite(cv) && isfinite(ref) && cv > 0 && ref > 0
 *     ratio = max(fl(cv / fl(ref + float32(1e-6))), 0)
 *
 * d_median[k] is the LOWER median of frame k's valid ratios, the value at index (count - 1) / 2 of their sorted sequence, which is
 * what torch.median returns; 1.0f where count = 0 (video_mvsa.py:292-293).  Where d_counts is not NULL, d_counts[k] = count.
 *
 * The median is exact and order-free.  A valid ratio is a non-negative float32 (+inf included, never a NaN), so the bit patterns
 * order as unsigned integers, and the median is selected by radix: four passes of 8 bits from the top, each a histogram of the
 * ratios that share the digits chosen so far -- counted in LDS and merged with integer atomics -- and a prefix walk that picks the
 * digit holding the sought index.  No sort, no floating-point atomic, nothing that depends on the launch geometry.  DECREE: the
 * reference computes on CUDA; the selection, the ratio and the choice of the lower median are torch's CPU kernels'.
 *
 * Workspace (1040 B per frame of a launch set: a histogram and the selection's state) comes from the context's pool and is bounded
 * by mdvt_config.workspace_mib: a large n_frames runs in launch sets.  The block follows the context's growth rule: a call that
 * needs more than any before waits for the device once before the smaller block is replaced.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL ctx, d_cv, d_ref or d_median; n_frames or any size of a given
 * plane < 1; a pitch below one row (4 * cv_w, 4 * ref_w, mask_w); with more than one frame a stride below rows * pitch; d_cv, d_ref,
 * their pitches and (more than one frame) strides, d_median or d_counts not a multiple of 4.  MDVT_ERR_UNSUPPORTED, likewise:
 * cv_w * cv_h >= 2^31.
 *
 * Footprint: exactly n_frames floats of d_median and, where given, n_frames words of d_counts; nothing else of the caller's.  The
 * result depends on no byte beyond the first 4 * cv_w, 4 * ref_w or mask_w of each row. */
int mdvt_ratio_median(mdvt_ctx* ctx, int n_frames,
                      int cv_w, int cv_h, const float* d_cv, size_t cv_pitch, size_t cv_stride,
                      int ref_w, int ref_h, const float* d_ref, size_t ref_pitch, size_t ref_stride,
                      int mask_w, int mask_h, const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride,
                      float* d_median, uint32_t* d_counts,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
