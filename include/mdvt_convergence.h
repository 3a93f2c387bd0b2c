/* mdvt_convergence.h -- per-frame convergence depths on the device: the entry point of libmdvt_hip.so behind step 4 of the reference's
 * pipeline (movie_2_3D.py:408-419 calls find_convergence_depth.py), declared outside include/mdvt.h like the FFV1 decoder's.
 *
 * find_convergence_depth.py:53-80 takes, per frame of a depth video, the float32 mean of the depths under a mask video's white
 * pixels, or of all depths where there is no mask frame; its list is the --convergence_file of stereo_rerender.py.  The mean feeds a
 * curve fit, the convergence angle and the vertex positions, so the device gives the reference's float32 bit for bit: NumPy's own
 * order of summation, stated below.
 */
#ifndef MDVT_CONVERGENCE_H
#define MDVT_CONVERGENCE_H

#include <stddef.h>
#include <stdint.h>

#include "mdvt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For each of n_frames depth frames of `height` rows of `width` pixels of 3 bytes (depth_order 0: R, G, B; 1: B, G, R) at
 * d_depth + k * depth_stride + row * depth_pitch, the mean d_means[k] of
 *
 *     depth = float32(R << 24 | B << 16) / float32(255^4 / max_depth)                        (find_convergence_depth.py:56-60)
 *
 * over the selected pixels in row-major order.  The divisor is computed in double and rounded once; the division is one correctly
 * rounded float32 division.  This is NOT the decode of mdvt_decode_depth and the renders, which multiply by max_depth / 255^4 as
 * depth_frames_helper.py:21-23 does and give other bits.
 *
 * Selection.  Frame k < n_mask_frames has the mask frame at d_mask + k * mask_stride + row * mask_pitch (same width and height,
 * mask_order as depth_order): a pixel is selected when gray > 240, gray = (4899 R + 9617 G + 1868 B + 8192) >> 14, OpenCV's 8-bit
 * COLOR_BGR2GRAY (find_convergence_depth.py:66-69).  Frames k >= n_mask_frames -- the mask video has run out, or there is none
 * (d_mask NULL, n_mask_frames 0) -- select every pixel (find_convergence_depth.py:70-74).
 *
 * Order (find_convergence_depth.py:77, NumPy's float32 mean of the n selected values): consecutive chunks of 8192 values, the last
 * one shorter; each chunk summed by the pairwise routine pw(a, n) -- n < 8: r = 0, r += a[i] in order; 8 <= n <= 128: r[k] = a[k],
 * r[k] += a[i + k] for i = 8, 16, ... < n - n % 8, then ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the last n % 8
 * values in order; else n2 = n / 2, n2 -= n2 % 8, pw(a, n2) + pw(a + n2, n - n2) --; the chunk sums added one after the other
 * from 0; the total divided by float32(n).  All in float32.  A frame that selects nothing gives a quiet NaN
 * (find_convergence_depth.py:79-80).  d_counts[k], where d_counts is given, is n.
 *
 * The call only enqueues on `stream` (a hipStream_t; NULL = the default stream): no host read-back, no synchronisation.  width and
 * height are those of the video, independent of the size the context renders at.  The result is deterministic and independent of
 * the launch geometry (no floating-point atomics).
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL d_depth or d_means, a pitch below 3 * width, a stride below
 * height * pitch (more than one frame), n_frames < 1, n_mask_frames outside [0, n_frames] or > 0 with a NULL mask, max_depth <= 0,
 * an unknown order.  MDVT_ERR_UNSUPPORTED, likewise: width * height > 2^28.
 *
 * Footprint: exactly n_frames floats of d_means and, where given, n_frames words of d_counts; nothing else of the caller's.  The
 * result depends on no byte beyond the first 3 * width of each row.  Workspace (per frame of a launch set 4 B per chunk; with a mask
 * also about 2.2 B per pixel) comes from the context's pool and is bounded by mdvt_config.workspace_mib: a large batch runs in
 * launch sets. */
int mdvt_convergence_depths(mdvt_ctx* ctx, int width, int height,
                            const uint8_t* d_depth, size_t depth_pitch, size_t depth_stride, int depth_order,
                            const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride, int mask_order,
                            int n_frames, int n_mask_frames, double max_depth, float* d_means, uint32_t* d_counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
