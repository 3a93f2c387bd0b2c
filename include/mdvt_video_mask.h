/* mdvt_video_mask.h -- the non-model work of the reference's mask-video step (generate_video_mask.py, step 3 of movie_2_3D.py) on the
 * device: the three entry points of libmdvt_hip.so behind tools/generate_video_mask.py, declared outside include/mdvt.h like the depth
 * engines'.
 *
 * The step is rembg's remove(only_mask=True) around a U2-Net: the frame is resized to the network's size and normalised, the network's
 * prediction is stretched to [0, 1], made bytes and resized to the frame's size.  Both resizes are Pillow's Image.resize(..., LANCZOS) on
 * 8-bit pixels.  Here are that resampler (mdvt_lanczos_resize_u8), the way into the network (mdvt_mask_model_input) and the way out of
 * it (mdvt_mask_from_prediction), so that a frame stays on the device from the decoder to the writer.
 *
 * All three calls only enqueue on `stream` (a hipStream_t; NULL = the default stream): no read-back, no synchronisation but the one a
 * scratch block may need when it grows (below).  Pitches and strides are in bytes and 64-bit.  The results do not depend on the launch
 * geometry; there are no floating-point atomics (a frame's maximum byte and a plane's minimum and maximum are taken with integer
 * atomics, which are exact and order-free).  The kernels are compiled with -ffp-contract=off and IEEE division.
 *
 * THE RESAMPLER (Pillow's Resample.c, 8 bits per channel, filter support 3).  Per axis, `in` samples to `out` samples, all in double:
 *
 *     scale = in / out;  fs = max(scale, 1.0);  support = 3.0 * fs;  ksize = 2 * (int)ceil(support) + 1
 *     for xx in 0 .. out-1:
 *         center = (xx + 0.5) * scale
 *         xmin = max((int)(center - support + 0.5), 0);   xmax = min((int)(center + support + 0.5), in) - xmin
 *         w[x] = L((x + xmin - center + 0.5) * (1.0 / fs))   for x in 0 .. xmax-1
 *         L(t) = sinc(t) * sinc(t / 3) for -3 <= t < 3, else 0;   sinc(0) = 1, sinc(t) = sin(pi t) / (pi t)   (M_PI, the C library's sin)
 *         ww = w[0] + w[1] + ... in sequence;   w[x] /= ww   (where ww != 0)
 *         k[x] = (int)(w[x] * 2^22 + (w[x] < 0 ? -0.5 : 0.5))         truncation toward zero
 *     out[xx] = clamp(((1 << 21) + sum_x in[xmin + x] * k[x]) >> 22, 0, 255)   int32, arithmetic shift
 *
 * The horizontal pass runs first, into a uint8 image of in_h rows; the vertical pass runs on that image.  A pass whose sizes are equal
 * is skipped.  Channels are independent.  The tables are built on the host (Pillow calls the C library's sin, and a device sin is not
 * promised to give its bits), once per (in, out) pair, and kept with the context; where a table is built the library checks that
 * 255 * sum|k| + 2^21 < 2^31 for every output, so the int32 sum cannot overflow.  This is OBSERVED: Pillow 12.2.0 is importable where
 * this library is built, and tests/video_mask_ref.py, the restatement the device is held to bit for bit, equals Image.resize byte for
 * byte on every case of tests/test_video_mask_cpu.py.  Where this text and Pillow disagree, Pillow is right.
 *
 * Two forms give the same bits.  FUSED: one workgroup per frame and strip of 8 output columns does the horizontal pass of the strip
 * into LDS (in_h * 8 * channels bytes) and the vertical pass out of it; the intermediate image never exists in global memory.  It needs
 * both passes and in_h * 8 * channels <= 65536.  TWO LAUNCHES: the horizontal pass into a workspace block, the vertical pass out of it;
 * a single pass goes straight from the input to the output.  The library's choice is two launches: measured on 16 frames of 1920 x 1080
 * and on 8 of 3840 x 2160, both to 320 x 320, the fused form took about twice as long (profiles/r19_video_mask.md).  It runs where
 * a caller asks for it.
 *
 * Workspace (the two-launch form's intermediate image, and what the two mask calls keep per frame) comes from the context's pool and
 * is bounded by mdvt_config.workspace_mib: a large batch runs in launch sets.  The blocks follow the context's growth rule: a call that
 * needs more than any before waits for the device once before the smaller block is replaced.  The tables are uploaded on the call's
 * stream when the call's size pairs are not the ones already on the device.  The host keeps the tables of up to 32 pairs; the call that
 * brings another waits for its stream once and starts over.  As for every entry point with a scratch block: ONE stream per ctx at a time.
 *
 * Size limit of all three: every width and height at most 8192 (MDVT_ERR_UNSUPPORTED beyond).
 */
#ifndef MDVT_VIDEO_MASK_H
#define MDVT_VIDEO_MASK_H

#include <stddef.h>
#include <stdint.h>

#include "mdvt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDVT_LANCZOS_AUTO 0        /* the library's choice (above) */
#define MDVT_LANCZOS_FUSED 1
#define MDVT_LANCZOS_TWO_LAUNCH 2

/* Image.resize((out_w, out_h), LANCZOS) on n_frames frames of in_h rows of in_w pixels of `channels` interleaved bytes (1: mode L;
 * 3: RGB or BGR, the order is irrelevant) at d_in + k * in_stride + row * in_pitch.  Output: uint8 frames of out_h rows of out_w
 * pixels of the same channel count at d_out + k * out_stride + row * out_pitch.  Equal sizes give a copy.
 *
 * form: MDVT_LANCZOS_AUTO, or the form to take.  Where h_form (host memory) is not NULL, an accepted call stores the form it took
 * there before it returns: MDVT_LANCZOS_FUSED, MDVT_LANCZOS_TWO_LAUNCH (a single pass too), or 0 where both passes were skipped.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL ctx, d_in or d_out; any of in_w, in_h, out_w, out_h, n_frames
 * < 1; channels not 1 or 3; form not 0, 1 or 2; in_pitch below channels * in_w, out_pitch below channels * out_w; with more than one
 * frame a stride below rows * pitch.  MDVT_ERR_UNSUPPORTED, likewise: a width or height above 8192; form MDVT_LANCZOS_FUSED where
 * that form does not exist (a skipped pass, or in_h * 8 * channels > 65536).
 *
 * Footprint: exactly the first channels * out_w bytes of each output row; nothing else of the caller's.  The result depends on no byte
 * beyond the first channels * in_w of each input row. */
int mdvt_lanczos_resize_u8(mdvt_ctx* ctx, int in_w, int in_h, int channels, int n_frames,
                           const uint8_t* d_in, size_t in_pitch, size_t in_stride,
                           int out_w, int out_h,
                           uint8_t* d_out, size_t out_pitch, size_t out_stride,
                           int form, int* h_form,
                           void* stream);

/* rembg's normalize (sessions/base.py) for n_frames packed frames of 3 bytes per pixel (order 0: R, G, B; 1: B, G, R) at d_frames
 * + k * frames_stride + row * frames_pitch:
 *
 *   1. the frame is resized to (model_w, model_h) as above (the library's choice of form);
 *   2. m = the RESIZED frame's maximum byte over all three channels; m = 0 is replaced by the double 1e-6 (max(np.max(im), 1e-6));
 *   3. value (k, c, y, x) of the planar float32 tensor [n_frames, 3, model_h, model_w], planes in R, G, B order whatever the input's,
 *      at d_out + k * out_stride + c * out_plane_stride + y * out_pitch + 4 * x, is float32((double(v) / m - mean[c]) / std[c]): two
 *      IEEE double divisions and one rounding to float32 (NumPy's uint8 / uint8 is float64).  h_mean and h_std are three host doubles
 *      each, in R, G, B order, read before the call returns.  U2-Net: (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), 320 x 320.
 *
 * DECREE.  rembg is not available where this library is built: steps 2 and 3 are stated from its source, not observed.  The tests hold
 * them to the NumPy expressions written out above.
 *
 * The device makes a table of 3 x 256 floats per frame and looks every byte up.  A thread takes four neighbouring pixels: four values
 * of a plane are one 16-byte store where d_out, out_pitch, out_plane_stride and out_stride are multiples of 16, element by element
 * otherwise and for the last one to three pixels of a row.  Both ways give the same bits.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL ctx, d_frames, d_out, h_mean or h_std; any of in_w, in_h,
 * model_w, model_h, n_frames < 1; order not 0 or 1; a mean or std that is not finite, a std of 0; frames_pitch below 3 * in_w,
 * out_pitch below 4 * model_w; out_plane_stride below model_h * out_pitch; with more than one frame frames_stride below
 * in_h * frames_pitch or out_stride below 3 * out_plane_stride; d_out, out_pitch, out_plane_stride or (more than one frame)
 * out_stride not a multiple of 4.  MDVT_ERR_UNSUPPORTED, likewise: a width or height above 8192.
 *
 * Footprint: exactly the first 4 * model_w bytes of each row of each plane; nothing else of the caller's.  The result depends on no
 * byte beyond the first 3 * in_w of each input row. */
int mdvt_mask_model_input(mdvt_ctx* ctx, int in_w, int in_h, int n_frames,
                          const uint8_t* d_frames, size_t frames_pitch, size_t frames_stride, int order,
                          int model_w, int model_h, const double* h_mean, const double* h_std,
                          float* d_out, size_t out_pitch, size_t out_plane_stride, size_t out_stride,
                          void* stream);

/* The tail of rembg's predict (sessions/u2net.py) and the mask video's frame, for n_frames float32 planes of pred_h rows of pred_w
 * values at d_pred + k * pred_stride + row * pred_pitch.  Per frame, in float32, each step rounded (fl):
 *
 *   1. mi, ma = the plane's minimum and maximum;
 *   2. p = fl(fl(x - mi) / fl(ma - mi)), one IEEE division;  b = (uint8) trunc(fl(p * 255.0f));
 *   3. the byte plane is resized to (out_w, out_h) as above, mode L (the library's choice of form);
 *   4. out_channels 1: one byte per pixel; 3: the byte three times, which is save_grayscale_video's frame with max_depth 255 (its
 *      clip / 255.0 * 255.0 and astype(uint8) are the identity on all 256 values).
 *      Frame k is at d_mask + k * mask_stride + row * mask_pitch.
 *
 * DECREES.  Steps 1 and 2 are stated from rembg's source, not observed.  A frame with ma == mi gives an all-zero mask (NumPy divides 0
 * by 0 there and casts a NaN, which is undefined).  A plane that holds a NaN or an infinity, or whose fl(ma - mi) is infinite, has no
 * defined result in the reference either: it is treated like ma == mi, an all-zero mask.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL ctx, d_pred or d_mask; any of pred_w, pred_h, out_w, out_h,
 * n_frames < 1; out_channels not 1 or 3; pred_pitch below 4 * pred_w, mask_pitch below out_channels * out_w; with more than one frame
 * a stride below rows * pitch; d_pred, pred_pitch or (more than one frame) pred_stride not a multiple of 4.
 * MDVT_ERR_UNSUPPORTED, likewise: a width or height above 8192.
 *
 * Footprint: exactly the first out_channels * out_w bytes of each row of d_mask; nothing else of the caller's.  The result depends on
 * no byte beyond the first 4 * pred_w of each input row. */
int mdvt_mask_from_prediction(mdvt_ctx* ctx, int pred_w, int pred_h, int n_frames,
                              const float* d_pred, size_t pred_pitch, size_t pred_stride,
                              int out_w, int out_h, int out_channels,
                              uint8_t* d_mask, size_t mask_pitch, size_t mask_stride,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif
