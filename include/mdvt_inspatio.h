/* mdvt_inspatio.h -- the alignment of the reference's InSpatio-World infill step (inspatio_world_infill.py, iwi:) on the device:
 * the 4 x 4 grid of masked cross-correlation shifts between a rendered eye and the video model's frame of it (iwi:76-115, 154-168),
 * declared outside include/mdvt.h like the scene detector's entry point.
 *
 * The reference calls scikit-image's phase_cross_correlation with a reference mask.  That function evaluates six correlation sums by
 * FFT in the images' float type and never rounds them.  Here the images are 8-bit grey under a 0/1 mask, so the six sums are integers
 * below 2^53: THE EXACT INTEGER SUMS AND THE FLOAT64 FORMULA BELOW ARE THIS PROJECT'S DEFINITION (DECREE), independent of any FFT
 * library, of the order of summation and of scikit-image's float type.
 *
 * RESTATED, NOT OBSERVED: scikit-image is not available where this was written.  The tolerance 1000 * eps of float32, the overlap
 * ratio 0.3, the clip to [-1, 1], the mean over tied maxima and the sign of the result are written from memory of its
 * cross_correlate_masked and _masked_phase_cross_correlation.  The sign is held by a test that needs no scikit-image
 * (tests/test_inspatio_cpu.py): an infilled frame that shows the render from three rows further down gives (3, 0), and warping by it
 * gives the render back.  The order of summation of the one-dimensional case is this project's (DECREE).
 */
#ifndef MDVT_INSPATIO_H
#define MDVT_INSPATIO_H

#include <stddef.h>
#include <stdint.h>

#include "mdvt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDVT_SHIFT_PATH_AUTO 0
#define MDVT_SHIFT_PATH_DIRECT 1
#define MDVT_SHIFT_PATH_TRANSFORM 2

/* For n_frames frames of one eye of `height` rows of `width` pixels: the blacked render R (3 bytes per pixel: R, G, B) at
 * d_render + k * render_stride + row * render_pitch, the model's frame I likewise at d_infilled, and the validity plane V (one byte
 * per pixel, non-zero = valid) at d_valid.  Written: d_shift[k][4][4][2] (float64: dy, then dx) and d_status[k][4][4] (uint8: 1 where
 * the cell's shift was computed, else 0 with a shift of +0.0, +0.0).
 *
 * Grey images: gR, gI = (4899 R + 9617 G + 1868 B + 8192) >> 14 (OpenCV's 8-bit COLOR_RGB2GRAY).
 * Cells: y_edges[g] = g * height / 4, x_edges[g] = g * width / 4 (integer division), g = 0 .. 4.  Cell (gy, gx) has h x w pixels of
 * which n are valid.  status = 0 where double(n) / double(h * w) < 0.2, and in a border column also where no row has a valid pixel.
 *
 * Interior columns (gx = 1, 2): for every displacement d = (dy, dx), |dy| <= h - 1, |dx| <= w - 1, over the pixels x of the cell
 * where V[x] and V[x - d] hold (x - d inside the cell too), with a = gI[x], b = gR[x - d]:
 *     N = sum 1, SF = sum a, SR = sum b, FR = sum a b, FF = sum a a, RR = sum b b            -- exact integers
 * Then in float64, every operation rounded once (no fused multiply-add, IEEE division and square root):
 *     N == 0: num = den = 0;  else num = FR - (SF * SR) / N,  fd = max(FF - (SF * SF) / N, 0),  rd = max(RR - (SR * SR) / N, 0),
 *                                  den = sqrt(fd * rd)
 *     tol = 1000 * 2^-23 * max over d of den
 *     c = den > tol ? min(max(num / den, -1), 1) : 0;   c = 0 where N < 0.3 * max over d of N
 *     m = max over d of c;   shift = (-(sum of d over all d with c == m)) / (their number), per axis: integer sums, one division.
 *
 * Border columns (gx = 0, 3): the same over dy alone (dx = 0) on row means.  Per row y of the cell, n_y = its valid pixels,
 * cnt = float32(n_y), or float32(1e-8) where n_y = 0; r[y] = fl32(fl32(sum of gR over the row's valid pixels) / cnt), q[y] likewise
 * of gI; a row counts where n_y > 0.  With a = q[y], b = r[y - dy] over the rows y where row y and row y - dy count, in ascending y,
 * one float64 accumulator per sum (a product of two float32 values is exact in float64).
 *
 * How the integer sums are made.  path = MDVT_SHIFT_PATH_AUTO takes what mdvt_masked_shift_path names for the eye's size;
 * MDVT_SHIFT_PATH_DIRECT sums them in integers, a thread per displacement, the cell in LDS; MDVT_SHIFT_PATH_TRANSFORM takes three
 * complex float64 transforms of the zero-padded cell (radix-2 passes in LDS; a + i a^2, b - i b^2 and V), their products, three
 * inverse transforms and rint.  Where d_round_error is given, its 8 bytes take the float64 bits of the largest |x - rint(x)| the
 * call rounded (0.0 on the direct path): the sums are exact while it stays below 0.5; tests hold it below 0.25.
 *
 * The call only enqueues on `stream` (a hipStream_t; NULL = the default stream): no host read-back.  No floating-point atomics: the
 * maxima are integer maxima of order-preserving keys, the index sums integer sums, so the result is independent of the launch geometry.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL d_render, d_infilled, d_valid, d_shift or d_status; a d_shift
 * or d_round_error that is not 8-byte aligned; n_frames < 1; width or height < 1; render_pitch or infilled_pitch below 3 * width,
 * valid_pitch below width; a stride below height * pitch (more than one frame); an unknown path.  MDVT_ERR_UNSUPPORTED, likewise: an
 * eye below 8 x 8; a cell side above 1024 (width or height above 4096); more than 2^24 frames; MDVT_SHIFT_PATH_DIRECT with a
 * largest cell of more than 16384 pixels (it does not fit the LDS).
 *
 * Footprint: n_frames * 32 float64 of d_shift, n_frames * 16 bytes of d_status, 8 bytes of d_round_error; nothing else of the
 * caller's.  Workspace: one scratch block of the context: 64 bytes per cell, and per interior cell of a launch set three complex
 * float64 planes (transform: of the padded size, 24 MiB for a 270 x 240 cell; direct: (2 h - 1) x (2 w - 1)).  The launch sets are
 * sized by mdvt_config.workspace_mib (0 = 4096 MiB), with ONE INTERIOR CELL AS THE FLOOR: a set never holds less than one cell's
 * planes, whatever the bound (192 MiB for a 1024 x 1024 cell).  The cells' state, 1 KiB per frame of the call, lies outside that
 * bound too: 225 KiB for a chunk. */
int mdvt_masked_shift_grid(mdvt_ctx* ctx, int width, int height, int n_frames,
                           const uint8_t* d_render, size_t render_pitch, size_t render_stride,
                           const uint8_t* d_infilled, size_t infilled_pitch, size_t infilled_stride,
                           const uint8_t* d_valid, size_t valid_pitch, size_t valid_stride,
                           int path, double* d_shift, uint8_t* d_status, uint64_t* d_round_error, void* stream);

/* The path MDVT_SHIFT_PATH_AUTO takes for an eye of this size: MDVT_SHIFT_PATH_DIRECT where its largest cell,
 * ceil(width / 4) x ceil(height / 4), has at most 4096 pixels, else MDVT_SHIFT_PATH_TRANSFORM; 0 where the size is refused.  A pure
 * function of its arguments: touches no device. */
int mdvt_masked_shift_path(int width, int height);

/* The alignment's warp (iwi:181-194): for n_frames frames of `height` rows of `width` pixels of 3 bytes at
 * d_infilled + k * infilled_stride + row * infilled_pitch, the flow grids d_grids[k][4][4][2] (float32: dx, then dy; device memory,
 * as inspatio_world.flow_grids makes them) and one byte per frame d_has_grid[k], the aligned frames at d_out, one pass per pixel:
 *     flow_dx, flow_dy = cv2.resize(grid[..., k], (width, height), INTER_LINEAR) on float32 at the pixel: THE FLOAT32 RESIZE of
 *         include/mdvt_metric_align.h (its index and weight tables, the horizontal pass, then the vertical), an enlargement from 4 x 4;
 *     map_x = fl32(float(x) - flow_dx), map_y = fl32(float(y) - flow_dy);
 *     cv2.remap(INTER_LINEAR, BORDER_REPLICATE) in OpenCV's fixed-point path as mdvt_equirect_remap states it: sx = rint(map_x * 32)
 *         (a tie to the even integer), ix = sx >> 5, fx = sx & 31, likewise y; the weights (32 - fx)(32 - fy) 32, fx (32 - fy) 32,
 *         (32 - fx) fy 32, fx fy 32 (sum 2^15); the result (sum + 2^14) >> 15 per channel -- with the four taps' coordinates clamped to
 *         the image where that call reads black.
 * A frame whose d_has_grid byte is 0 is copied.  A NaN or an out-of-range flow reads some pixel of the frame (the clamps hold).
 * d_out must not overlap d_infilled.  RESTATED, NOT OBSERVED, as the two restatements it is built from.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: a NULL buffer, a d_grids that is not 4-byte aligned, width, height or
 * n_frames < 1, a pitch below 3 * width, a stride below height * pitch (more than one frame).  MDVT_ERR_UNSUPPORTED: width * height
 * >= 2^31.  Footprint: the first 3 * width bytes of every row of d_out; no workspace.  Only enqueues on `stream`. */
int mdvt_flow_warp(mdvt_ctx* ctx, int width, int height, int n_frames, const float* d_grids, const uint8_t* d_has_grid,
                   const uint8_t* d_infilled, size_t infilled_pitch, size_t infilled_stride,
                   uint8_t* d_out, size_t out_pitch, size_t out_stride, void* stream);

/* The step's frame preparation (iwi:385-426, 279-301) for one eye of n_frames side-by-side frames: d_color and d_mask hold rows of
 * 2 * eye_w pixels of 3 bytes (the render and the infill mask; rows at the pitches, frames at the strides); eye 0 is the left half, 1
 * the right; nothing is mirrored.  Written per frame:
 *     d_valid         V, eye_h rows of eye_w bytes: 255 where all three mask bytes are 0, else 0
 *     d_render        the eye's render with every pixel where V == 0 set to black (3 bytes per pixel)
 *     d_model_render  d_render through THE U8 RESIZE of include/mdvt_infill_adapter.h (cv2.resize(INTER_LINEAR) on uint8, restated;
 *     d_model_valid   its equal-size copy and exact 2 x area mean included: the same device code) to model_w x model_h, and V
 *                     likewise, resized as a one-channel image and NOT thresholded
 *     d_hole_counts   one uint32 per frame: the pixels with V == 0
 * The call only enqueues on `stream`.  MDVT_ERR_INVALID_ARG, before anything is launched or written: a NULL buffer, a d_hole_counts
 * that is not 4-byte aligned, a size or n_frames < 1, an eye other than 0 and 1, an input pitch below 6 * eye_w, an output pitch below
 * its row, a stride below its frame (more than one frame).  MDVT_ERR_UNSUPPORTED: an image of 2^31 pixels or of more than 65535 rows.
 * Footprint: the rows' own bytes of the four images and n_frames words of d_hole_counts; no workspace. */
int mdvt_inspatio_prepare_eye(mdvt_ctx* ctx, int eye_w, int eye_h, int n_frames, int eye,
                              const uint8_t* d_color, size_t color_pitch, size_t color_stride,
                              const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride, int model_w, int model_h,
                              uint8_t* d_valid, size_t valid_pitch, size_t valid_stride,
                              uint8_t* d_render, size_t render_pitch, size_t render_stride,
                              uint8_t* d_model_valid, size_t model_valid_pitch, size_t model_valid_stride,
                              uint8_t* d_model_render, size_t model_render_pitch, size_t model_render_stride,
                              uint32_t* d_hole_counts, void* stream);

/* The second form: n_frames frames of in_w x in_h pixels of 3 bytes through THE U8 RESIZE to model_w x model_h -- the original
 * colour frames to the model's size (iwi:436-437), and the model's frames back to the eye's.  Refusals as above. */
int mdvt_inspatio_model_frames(mdvt_ctx* ctx, int in_w, int in_h, int n_frames, const uint8_t* d_frames, size_t frames_pitch, size_t frames_stride,
                               int model_w, int model_h, uint8_t* d_out, size_t out_pitch, size_t out_stride, void* stream);

/* The step's compositing (iwi:481-518) for one eye of n_frames frames: d_aligned holds the aligned frames at the eye's size (3 bytes
 * per pixel), d_color and d_mask the side-by-side render and infill mask (rows of 2 * eye_w pixels), d_pasted and d_blended
 * side-by-side frames of which the eye's half is written; eye 0 is the left half, 1 the right; nothing is mirrored.
 *     hole    = a mask byte of the pixel is not 0
 *     pasted  = hole ? aligned : render                            (it feeds the chunk overlap)
 * and, where d_blended is given (--apply_edge_blending):
 *     alpha   = mark_lower_side of the eye's mask image, as mdvt_mark_lower_side marks it in 30 steps, grown by three 4-neighbour
 *               dilations with the border as background (a pixel within L1 distance 3 of a mark), as a 0 / 1 float32 plane through
 *               cv2.GaussianBlur(., (5, 5), 0) with BORDER_REFLECT_101: OpenCV's fixed table for size 5 and sigma 0,
 *               1/16 4/16 6/16 4/16 1/16 per axis.  On a 0 / 1 plane every product and sum is exact in float32, so alpha has one
 *               set of bits whatever the order
 *     blended = trunc(clip(fl(fl(alpha * aligned) + fl(fl(1 - alpha) * pasted)), 0, 255)) per channel, in float32
 * The structure is mdvt_adapter_composite_eye's without its resize and mirroring; the march is the same device code
 * (launch_mark_lower_side), and that call's bytes are unchanged.  RESTATED, NOT OBSERVED: the Gaussian's table (no OpenCV here).
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: a NULL d_aligned, d_color, d_mask or d_pasted, a size or n_frames
 * < 1, an eye other than 0 and 1, aligned_pitch below 3 * eye_w, another pitch below 6 * eye_w, a stride below its frame (more than
 * one frame).  MDVT_ERR_UNSUPPORTED: an eye below 8 x 8 or of more than 65535 rows; a mask frame beyond the march's 32-bit offsets.
 * Footprint: the eye's half of the rows of d_pasted and d_blended.  Workspace (blending): the context's adapter scratch block, one
 * frame at a time.  Only enqueues on `stream`. */
int mdvt_inspatio_composite_eye(mdvt_ctx* ctx, int eye_w, int eye_h, int n_frames, int eye,
                                const uint8_t* d_aligned, size_t aligned_pitch, size_t aligned_stride,
                                const uint8_t* d_color, size_t color_pitch, size_t color_stride,
                                const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride,
                                uint8_t* d_pasted, size_t pasted_pitch, size_t pasted_stride,
                                uint8_t* d_blended, size_t blended_pitch, size_t blended_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif
