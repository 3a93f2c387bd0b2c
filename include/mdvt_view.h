/* mdvt_view.h -- the free-camera viewer's device work: the entry points of libmdvt_hip.so behind the reference's
 * 3d_view_depthfile.py --render (3dv:133-258; dmt = depth_map_tools.py), declared outside include/mdvt.h like the convergence depths'.
 *
 * The tool draws every frame of a depth video from a camera placed at --x --y --z that looks at a target, by default the centre of
 * the frame's own geometry: `lookat = draw_mesh.get_center()` (3dv:231), the mean of the frame's transformed vertices.  That mean is
 * mdvt_view_centers below.  The image is mdvt_render_view_batch: one image per frame from the composed matrix V * T_frame, with the
 * holes left in the key colour (3dv:254 writes the render as it comes; the tool's key is white).
 *
 * Two decrees of this interface (DESIGN.md section 5.8 gives the reasons), and a third the render shares with the stereo path (the
 * near-plane decree of DESIGN.md section 3):
 *   - the order of the centre's sums is NumPy's, not Open3D's (below);
 *   - the camera is where the flags say: the view matrix the project renders with has its rows [r, -r.p], [u, -u.p], [f, -f.p],
 *     (0, 0, 0, 1) for f = (t - p) / |t - p|, r = cross((0, 1, 0), f) / |.|, u = cross(f, r) (x right, y down, z forward).  What Open3D
 *     makes of the matrix of dmt:1618-1638 -- its rotation transposed, the position with a negated z in the last column, a last row
 *     that is not (0, 0, 0, 1) -- cannot be observed without Open3D; metric_depth_video_toolbox_amd/view_depthfile.py restates that
 *     function for completeness and does not render with it.
 */
#ifndef MDVT_VIEW_H
#define MDVT_VIEW_H

#include <stddef.h>
#include <stdint.h>

#include "mdvt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* draw_mesh.get_center() of 3dv:231 for each of n_frames frames of the context's W x H: d_centers[3 k .. 3 k + 2] (DEVICE, f64,
 * 8-byte aligned) = the mean x, y, z of frame k's N = W H vertices.  params: HOST array of n_frames; the depth frame k lies at
 * d_depth_rgb + k * depth_stride + row * depth_pitch (u8 RGB-coded depth, as mdvt_io.depth_rgb).  The context's config supplies
 * mode, remove_edges and max_depth.  Of params[k] the call reads K, depth_scale, has_T and T (Krender is validated as the render
 * calls validate it; convergence_angle is ignored).
 *
 * Vertices (3dv:164, 182; dmt:1112-1133 as NumPy >= 2 evaluates it): depth = f32(code) * f32(max_depth / 255^4), then * f32(depth_scale)
 * in f32; widened to f64; x = ((gx - cx) * z) / fx, y = ((gy - cy) * z) / fy, z -- gx, gy the integer grid in points mode and the
 * f32 grid f32(j) * f32((W + 1) / W), f32(i) * f32((H + 1) / H) in mesh mode (of_by_one, 3dv:178-180).
 * Pose (3dv:185-186), with has_T: Open3D's point transform in f64 -- h_r = ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3] * 1 for
 * the four rows, then x, y, z = h_0 / h_3, h_1 / h_3, h_2 / h_3.  T must be affine as the render calls require.
 * Parked vertices (3dv:195-196, dmt:1091): in points mode with remove_edges the vertices of the triangles that the 89-degree filter
 * removes (the filter of mdvt_edge_filter, on the integer grid as the render of that mode runs it) are replaced AFTER the pose by
 * (-0.2, -0.2, -0.2).  In mesh mode they stay where they are.
 * Mean: center[c] = S_c / f64(N), S_c = np.sum of the contiguous f64 array of coordinate c over the N vertices in row-major order:
 * consecutive chunks of 8192 values, each summed by the pairwise routine that include/mdvt_convergence.h states (here in f64), the
 * chunk sums added one after the other from 0.
 *
 * That order is a DECREE.  Open3D's get_center adds the vertices one after the other, which no parallel sum reproduces; NumPy's order
 * is one a device can give bit for bit, and it is the more accurate of the two.  For either order the error of S_c is at most
 * (N - 1) * 2^-53 * sum |v|, so the two centres differ by at most 2 (N - 1) * 2^-53 * sum |v| / N: 1.5e-8 m for a 3840 x 2160
 * frame of the benchmark's scene, where 6e-12 m was measured (profiles/r15_view_centers.md) -- nothing a pixel of the view can show.
 *
 * The call only enqueues on `stream` (a hipStream_t; NULL = the default stream): no host read-back.  It waits for the device only
 * when its workspace has to grow (the first call, or a larger one than before).  The result is deterministic and independent of the
 * launch geometry and of the workspace's size (no floating-point atomics).
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: no config set, NULL params, d_depth_rgb or d_centers, d_centers not
 * 8-byte aligned, n_frames < 1, depth_pitch below 3 W, depth_stride below H * depth_pitch (more than one frame), a frame below
 * 2 x 2 where vertices are parked, and what the render calls refuse of a frame's parameters (focal lengths, depth_scale <= 0).
 * MDVT_ERR_UNSUPPORTED, likewise: W * H > 2^28, a pose that is not affine, 2 cx != W or 2 cy != H of Krender.
 *
 * Footprint: exactly 3 * n_frames doubles of d_centers, nothing else of the caller's.  The result depends on no byte beyond the
 * first 3 W of each depth row.  All pitches, strides and frame offsets are 64-bit.  Workspace, from the context's pool under the one
 * growth rule of its scratch blocks: 24 B per chunk and frame of a launch set, with parking also 1 B per pixel; bounded by
 * mdvt_config.workspace_mib -- a large batch runs in launch sets. */
int mdvt_view_centers(mdvt_ctx* ctx, int n_frames, const mdvt_frame_params* params,
                      const uint8_t* d_depth_rgb, size_t depth_pitch, size_t depth_stride,
                      double* d_centers, void* stream);

/* Device buffers of a view render: mdvt_io with ONE image per frame.  *_pitch = bytes between rows, *_stride = bytes between frames,
 * all 64-bit.  mask, depth and hole_counts may be NULL. */
typedef struct mdvt_view_io {
    const uint8_t* depth_rgb;  size_t depth_pitch;  size_t depth_stride;   /* RGB-coded 16-bit depth              */
    const uint8_t* color_rgb;  size_t color_pitch;  size_t color_stride;   /* colour frame                        */
    uint8_t* rgb;   size_t rgb_pitch;  size_t rgb_stride;                  /* the image; holes hold cfg.key_rgb   */
    uint8_t* mask;  size_t mask_pitch; size_t mask_stride;                 /* optional: 255 = hole                */
    float* depth;   size_t zout_pitch; size_t zout_stride;                 /* optional: 0 = background; 4-byte aligned */
    uint32_t* hole_counts;                                                 /* optional: [n_frames], overwritten   */
} mdvt_view_io;

/* The render of 3dv:254 for n_frames frames: ONE image per frame, what the left eye of mdvt_render_stereo_batch gives with
 * ipd_m = 0, no convergence and T = params[k].T -- the same snap, fill rule, culling, tie rule and near-plane decree, held bit for
 * bit to the oracle's left eye (orc_render_stereo with ipd_m = 0) -- except that a hole pixel of rgb holds cfg.key_rgb instead of
 * black.  The mask keeps the colour-key rule (255 where nothing was drawn or the drawn colour equals the key).
 * params[k].T holds the composed world-to-camera matrix V_k * T_k, row major, and has_T must be 1: the library does no 4 x 4 product
 * (view_depthfile.view_params composes it with one NumPy product).  convergence_angle and cfg.ipd_m are ignored.
 * Mesh and points mode, remove_edges on and off (in points mode the vertices of removed triangles are not drawn, as in the stereo
 * path -- a stated departure: the reference would draw them as one pixel at V * (-0.2, -0.2, -0.2)), cull, both sub-pixel grids.
 * The work is one eye's: the one-eye instantiations of the general kernels (points splat and resolve; the mesh's cell walk, queue,
 * huge-triangle and tie passes) on eye 0's key planes of the context's workspace -- a context that renders only views allocates no
 * plane of a second eye --, in the launch sets and on the side stream of the stereo call for batches longer than a launch set.
 * Only enqueues on `stream`; waits for the device only when the workspace has to grow.  ONE stream per ctx at a time.
 * MDVT_ERR_UNSUPPORTED, before anything is written: cfg.edge_points != 0, samples = 4, near-plane clipping switched on (seed images
 * and packed mask bits have no field here), and what fill of a frame's parameters refuses (a pose that is not affine, Krender's size).
 * MDVT_ERR_INVALID_ARG, likewise: no config, NULL params / io / depth_rgb / color_rgb / rgb, has_T = 0, a pitch below one row, a
 * stride below one frame (more than one frame), a depth plane or hole counts that are not dword aligned, a frame below 2 x 2.
 * Footprint: the first 3 W bytes of each row of rgb, W of mask, 4 W of depth, n_frames words of hole_counts, nothing else of the
 * caller's; the result depends on no byte beyond the first 3 W of each input row. */
int mdvt_render_view_batch(mdvt_ctx* ctx, int n_frames, const mdvt_frame_params* params, const mdvt_view_io* io, void* stream);

#ifdef __cplusplus
}
#endif
#endif
