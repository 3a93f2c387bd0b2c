/* mdvt_scene.h -- scene detection on the device: the entry point of libmdvt_hip.so behind step 0 of the reference's pipeline
 * (movie_2_3D.py:209-222 runs PySceneDetect's `scenedetect -i movie list-scenes`), declared outside include/mdvt.h like the FFV1
 * decoder's.
 *
 * PySceneDetect's content detector scores a frame by the mean absolute difference of its hue, saturation and value planes to the
 * previous frame's.  The planes are integers, so the three sums of a frame pair are exact integers: the device gives those, 24 bytes
 * per frame, and metric_depth_video_toolbox_amd/scene_detect.py turns them into scores and cuts on the host in float64.
 */
#ifndef MDVT_SCENE_H
#define MDVT_SCENE_H

#include <stddef.h>
#include <stdint.h>

#include "mdvt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For n_frames frames of `height` rows of `width` pixels of 3 bytes (order 0: R, G, B; 1: B, G, R) at
 * d_frames + k * stride + row * pitch, and an optional previous frame d_prev (rows at prev_pitch, same size and order; NULL = none),
 * the sums of every consecutive pair: d_sums[3 p + 0 .. 2] = sum |dH|, sum |dS|, sum |dV| over the pixels of the analysed image.
 * The pairs are (prev, 0) where d_prev is given, then (0, 1) ... (n_frames - 2, n_frames - 1): n_frames - 1 + (d_prev != NULL) of
 * them.
 *
 * The analysed image.  factor == 1: the frame itself.  factor > 1: the frame through THE U8 RESIZE of include/mdvt_infill_adapter.h
 * (cv2.resize with INTER_LINEAR on uint8, including its exact 2 x area mean) to (rnd(width / factor), rnd(height / factor)), where
 * rnd rounds to the nearest integer and a tie to the even one (Python's round): q = n / factor, r = n % factor; q + 1 where
 * 2 r > factor, q + (q & 1) where 2 r == factor, else q.
 *
 * H, S, V of a pixel (r, g, b): OpenCV's 8-bit COLOR_BGR2HSV with H in [0, 180).
 *     v = max(r, g, b), m = min(r, g, b), d = v - m
 *     S = min(255, (d * sdiv[v] + 2048) >> 12)            sdiv[0] = 0, sdiv[i] = rint((255 << 12) / double(i))
 *     h = g - b where v == r, else b - r + 2 d where v == g, else r - g + 4 d
 *     H = (h * hdiv[d] + 2048) >> 12                      hdiv[0] = 0, hdiv[i] = rint((180 << 12) / (6.0 * i))
 *         (an arithmetic shift of a signed int), H += 180 where H < 0
 *     V = v
 * rint rounds a tie to the even integer.  |dH| is the plain difference of the two hues, not the distance on the circle.
 *
 * The sums are exact integers, 64 bits wide, and independent of the launch geometry (integer atomics; no floating point).
 *
 * The call only enqueues on `stream` (a hipStream_t; NULL = the default stream): no host read-back, no synchronisation.  width and
 * height are those of the video, independent of the size the context renders at.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL d_frames or d_sums, a d_sums that is not 8-byte aligned, a
 * pitch (or, with d_prev, prev_pitch) below 3 * width, a stride below height * pitch (more than one frame), n_frames < 1, no pair
 * (n_frames == 1 without d_prev), factor < 1 or a factor that leaves the analysed image without a row or a column, an unknown
 * order.  MDVT_ERR_UNSUPPORTED, likewise: width * height > 2^28.
 *
 * Footprint: exactly 3 * pairs 64-bit words of d_sums; nothing else of the caller's.  The result depends on no byte beyond the
 * first 3 * width of each row.  No workspace. */
int mdvt_scene_frame_sums(mdvt_ctx* ctx, int width, int height, int n_frames,
                          const uint8_t* d_frames, size_t pitch, size_t stride, int order,
                          const uint8_t* d_prev, size_t prev_pitch, int factor, uint64_t* d_sums, void* stream);

/* 1 where mdvt_scene_frame_sums reads such frames with 16-byte loads, 0 where it reads them byte by byte (the sums are the same):
 * factor == 1, and d_frames, pitch, the stride of more than one frame and, where given, d_prev and prev_pitch are multiples
 * of 16.  A pure function of its arguments: touches no device. */
int mdvt_scene_vector_path(int n_frames, const uint8_t* d_frames, size_t pitch, size_t stride,
                           const uint8_t* d_prev, size_t prev_pitch, int factor);

#ifdef __cplusplus
}
#endif
#endif
