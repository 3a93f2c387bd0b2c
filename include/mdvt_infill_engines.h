/* mdvt_infill_engines.h -- the frames around two more in-painting models on the device: the two entry points of libmdvt_hip.so behind
 * the reference's m2svid_infill.py:224-261 ("m2s") and stereo_dissoclusion_net_infill.py:100-123 ("sdn"), declared outside
 * include/mdvt.h like the infill adapter's (include/mdvt_infill_adapter.h), whose conventions they share.
 *
 * movie_2_3D.py's step 6 picks an --infill_engine.  `m2svid` feeds its model three inputs per eye -- the rendered eye, the original
 * frame and a coarse mask -- and pastes the model's frames back exactly as the StereoCrafter step does: mdvt_m2svid_prepare_eye makes
 * the inputs, mdvt_adapter_composite_eye (mdvt_infill_adapter.h) does the rest.  `stereo_dissoclusion_net` runs its model per frame at
 * the eye's own size and then finishes the way basic_nomal_infill.normal_infill does behind its marched fill: mdvt_model_infill_finish.
 * The models are the caller's.
 *
 * Both calls only enqueue on `stream` (a hipStream_t; NULL = the default stream), take 64-bit pitches and strides (bytes; frame k of an
 * array lies at base + k * stride, row y of a frame at + y * pitch; all address arithmetic is 64-bit) and refuse a bad layout with
 * MDVT_ERR_INVALID_ARG before anything is launched or written: a NULL ctx or buffer, a size or count below 1, a pitch below a row, a
 * stride below rows * pitch with more than one frame, a uint32 array that is not aligned to its element.  Images are u8 RGB, three
 * bytes per pixel.  The outputs may not overlap the inputs.
 *
 * THE U8 RESIZE is the one mdvt_infill_adapter.h states: cv2.resize(src, (out_w, out_h)) (INTER_LINEAR) on uint8 as OpenCV's plain
 * C++ path has it -- the linear path, the copy at equal sizes and the 2 x 2 area mean at exactly half the size -- RESTATED, not observed
 * (there is no OpenCV where the library is built).  No byte parity with cv2 is claimed for it.
 */
#ifndef MDVT_INFILL_ENGINES_H
#define MDVT_INFILL_ENGINES_H

#include <stddef.h>
#include <stdint.h>

#include "mdvt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* m2s:224-261.  The three model inputs of one eye of n_frames frames, in one launch set.  d_color, d_mask: side-by-side colour and
 * infill-mask frames of eye_h rows of 2 * eye_w pixels, as in mdvt_adapter_prepare_eye; d_org: the original colour frames of org_h rows
 * of org_w pixels; `eye` 0 = the left half read mirrored (np.fliplr), 1 = the right half as it is.  Per frame:
 *     d_image       the eye's half resized to image_w x image_h (the u8 resize)                                        m2s:234-236, 254-256
 *     d_org_image   the WHOLE original frame resized to image_w x image_h, mirrored for eye 0 likewise               m2s:239-241, 259-261
 *     d_model_mask  mask_h rows of mask_w bytes: the plane (any channel of the mask pixel != 0 ? 255 : 0) of that half, mirrored
 *                   likewise, resized to mask_w x mask_h, then > 0 -> 255, else 0                                     m2s:226-231, 244-251
 *     d_hole_counts one uint32 in DEVICE memory: the 255s written to that frame's mask (0 in every frame of a chunk: the reference
 *                   skips the model for that eye, m2s:271, 280)
 * The reference's sizes are image 512 x 512 and mask 64 x 64.  A thread makes one output pixel and reads the source pixels that pixel
 * needs, once.
 *
 * MDVT_ERR_INVALID_ARG also: eye not 0 or 1; color_pitch or mask_pitch below 6 * eye_w, org_pitch below 3 * org_w, image_pitch or
 * org_image_pitch below 3 * image_w, model_mask_pitch below mask_w.  MDVT_ERR_UNSUPPORTED, likewise before anything is written: image_h
 * or mask_h above 65535.
 *
 * Footprint: the first 3 * image_w bytes of each row of each image and each original image, the first mask_w bytes of each row of each
 * mask, the n_frames counts (every one is written: they may arrive poisoned); nothing else.  No workspace.  The result depends on no
 * byte outside the eye's 3 * eye_w bytes of each side-by-side row and the first 3 * org_w bytes of each original row. */
int mdvt_m2svid_prepare_eye(mdvt_ctx* ctx, int eye_w, int eye_h, int n_frames, int eye,
                            const uint8_t* d_color, size_t color_pitch, size_t color_stride,
                            const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride,
                            const uint8_t* d_org, int org_w, int org_h, size_t org_pitch, size_t org_stride,
                            int image_w, int image_h, int mask_w, int mask_h,
                            uint8_t* d_image, size_t image_pitch, size_t image_stride,
                            uint8_t* d_org_image, size_t org_image_pitch, size_t org_image_stride,
                            uint8_t* d_model_mask, size_t model_mask_pitch, size_t model_mask_stride,
                            uint32_t* d_hole_counts, void* stream);

/* sdn:100-123, everything after the model, for n_images images of height rows of width pixels.  d_img: the eye as rendered; d_model:
 * the model's image for it; d_infill_mask: the finished infill-mask image (normal-coloured).  In the reference's order:
 *     bg(p)   = every channel of the mask pixel is non-zero                                                           sdn:101
 *     B       = cv2.blur(model, (4, 4)): anchor (2, 2), BORDER_REFLECT_101, cvRound (half to even), as mdvt_normal_infill restates it   sdn:108
 *     work    = bg ? B : img                                                                                          sdn:111
 *     grown   = mark_lower_side(mask, 30 steps) as mdvt_mark_lower_side, the marks grown by six 4-neighbour dilations (scipy's
 *               binary_dilation(iterations=6): the image border is background)                                        sdn:115-119
 *     out     = grown ? the 6 x 6 Gaussian of work over the grown pixels only (blur_under_mask, sdn:50-90, line for line the function
 *               at basic_nomal_infill.py:45-85 that mdvt_normal_infill restates) : work                               sdn:122
 * This is the tail of mdvt_normal_infill with the marched fill replaced by a dense image that somebody else made; it runs on that
 * call's listed-pixel stages: one dense pass copies the image and lists the pixels with a non-black mask, and the box mean (bg pixels
 * only), the march, the diamond growth and the Gaussian (grown pixels only) work on lists.  A non-black mask pixel with a zero channel
 * marches for the lower side but is not bg.  The Gaussian's bits and cv2.blur's are RESTATED, not observed, as for mdvt_normal_infill.
 *
 * MDVT_ERR_INVALID_ARG also: a pitch below 3 * width; d_out equal to an input.  MDVT_ERR_UNSUPPORTED, before anything is written:
 * the marches' limits mask_pitch >= 2^24 or mask_pitch * height >= 2^32; height > 65535.
 *
 * Workspace: a scratch block of the context (the one mdvt_normal_infill uses: mdvt.h's rule of ONE stream per ctx at a time for the
 * calls with a library-owned workspace covers this call too), about 16 bytes per pixel (two pixel lists of about 4 bytes each, a 3-byte side image and
 * four byte planes, laid out as mdvt_normal_infill's) of each of the up to 16 images in flight, under the context's growth rule: the first call allocates it, and a
 * later call that needs more waits for the device once (hipDeviceSynchronize) before the smaller block is replaced; a call that
 * needs no more than an earlier one never waits.
 *
 * Footprint: the first 3 * width bytes of each row of each output image (every one is written); nothing else of the caller's.  The
 * result depends on no byte beyond the first 3 * width of each input row. */
int mdvt_model_infill_finish(mdvt_ctx* ctx, int width, int height, int n_images,
                             const uint8_t* d_img, size_t img_pitch, size_t img_stride,
                             const uint8_t* d_model, size_t model_pitch, size_t model_stride,
                             const uint8_t* d_infill_mask, size_t mask_pitch, size_t mask_stride,
                             uint8_t* d_out, size_t out_pitch, size_t out_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif
