/* mdvt_geometry.h -- geometry export: the entry points of libmdvt_hip.so behind the reference's
 * convert_metric_depth_video_to_other_format.py (cmf: below; dmt = depth_map_tools.py, dfh = depth_frames_helper.py), declared outside
 * include/mdvt.h like the viewer's.
 *
 * The exporter is the third caller of get_mesh_from_depth_map, after stereo_rerender.py and 3d_view_depthfile.py.  With --save_ply
 * and --save_obj it writes one point cloud or mesh per frame (cmf:692-749), with --bit8 and --bit16 a grey depth video (cmf:752-760).
 * The renders build the same geometry and keep it in registers; mdvt_export_geometry_batch materialises it: every vertex, the
 * triangles that survive the 89-degree filter in draw order, and the used vertices in index order.  mdvt_depth_grey_batch is the grey
 * depth.
 *
 * Decrees of this interface (DESIGN.md section 5.9 gives the reasons):
 *   - the lists are in the reference's own order and are produced by an ordered compaction (counts, a scan, a scatter in separate
 *     launches): no atomic's order shows in a result;
 *   - grey depth values beyond the type's range SATURATE (below);
 *   - the files the lists are written to (metric_depth_video_toolbox_amd/geometry_files.py) have this project's own layout: Open3D's
 *     exact bytes cannot be observed without Open3D.
 */
#ifndef MDVT_GEOMETRY_H
#define MDVT_GEOMETRY_H

#include <stddef.h>
#include <stdint.h>

#include "mdvt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mdvt_geometry_opts {
    int32_t decode;        /* 0 = the exporter's own (cmf:646-652), 1 = dfh's (dfh:63-75, 13-24: the render's) */
    int32_t remove_edges;  /* --remove_edges (cmf:692) */
    int32_t reserved[2];   /* 0 */
    double  max_depth;
} mdvt_geometry_opts;

/* Device buffers of an export.  All pitches / strides in bytes, 64-bit; a stride is the distance between two frames' lists.  Optional
 * outputs may be NULL.  N = W H of the context. */
typedef struct mdvt_geometry_io {
    const uint8_t* depth_rgb; size_t depth_pitch; size_t depth_stride;  /* RGB-coded depth                                      */
    const uint8_t* color_rgb; size_t color_pitch; size_t color_stride;  /* needed only for point_rgb                            */
    double*   vertices;   size_t vertices_stride;   /* [N][3] f64, every vertex, posed                      */
    int32_t*  triangles;  size_t triangles_stride;  /* [<= 2(H-1)(W-1)][3], kept triangles, draw order     */
    int32_t*  used_index; size_t used_stride;       /* [<= N] ascending indices of used vertices           */
    double*   points;     size_t points_stride;     /* [<= N][3] = vertices[used_index]                    */
    uint8_t*  point_rgb;  size_t point_rgb_stride;  /* [<= N][3] = colour of used vertices                 */
    uint32_t* counts;                               /* [n_frames][2] = {U used vertices, M kept triangles} */
} mdvt_geometry_io;

/* The geometry of cmf:692-749 for n_frames frames of the context's W x H: what get_mesh_from_depth_map (dmt:1205-1384), called as at
 * cmf:692 with its default of_by_one = True, hands the exporter, and what the exporter keeps of it.  params: HOST array of n_frames; of
 * params[k] the call reads K, depth_scale, has_T and T and nothing else.  The context's configuration is not read (max_depth and
 * remove_edges are the opts'), and none has to be set.
 *
 * Depth.  decode = 1: f32(code) * f32(max_depth / 255^4), code = R << 24 | B << 16, the render's multiply (dfh:21-23).  decode = 0:
 * code = ((R + G) >> 1) << 24 | B << 16 (cmf:648-649), then ONE correctly rounded f32 division by f32(255^4 / max_depth), as NumPy >= 2
 * evaluates cmf:652 -- the rule include/mdvt_convergence.h states.  Both are then * f32(depth_scale).
 * Vertices (dmt:1112-1133 with of_by_one): the f32 grid gx = f32(j) * f32((W + 1) / W), gy = f32(i) * f32((H + 1) / H); widened to f64:
 * x = ((gx - cx) * z) / fx, y = ((gy - cy) * z) / fy, z.  Exactly the vertex of the 89-degree filter and of include/mdvt_view.h.
 * Filter (dmt:1283-1294): mdvt_edge_filter's, on the unposed vertices; with remove_edges = 0 nothing is removed.
 * Kept triangles: the reference's triangles_all order (dmt:1243-1254) -- tri1 = (idx1, idx2, idx3) = (v[i][j], v[i+1][j], v[i+1][j+1])
 * of every cell in row-major order, then tri2 = (idx1, idx3, idx4) = (v[i][j], v[i+1][j+1], v[i][j+1]) of every cell -- with the removed
 * ones left out (cmf:737-739).  Indices refer to the full vertex array.
 * Used vertices (dmt:1378-1384, used_indices as returned to cmf:692): the vertices of at least one kept triangle, ascending.  NOT the
 * complement of mdvt_edge_filter's d_unused: a vertex can belong to a kept and to a removed triangle.  With remove_edges = 0: 0 .. N-1.
 * Pose (cmf:694-695), with has_T: Open3D's point transform in f64 as include/mdvt_view.h states it -- h_r = ((T[r][0] x + T[r][1] y) +
 * T[r][2] z) + T[r][3] * 1 for the four rows, then x, y, z = h_0 / h_3, h_1 / h_3, h_2 / h_3 -- applied after the filter, to `vertices`
 * and `points` alike.  T must be affine as the render calls require.
 * point_rgb[u] = the three bytes of color_rgb at vertex used_index[u] (cmf:746: byte / 255.0 goes back to the same byte).
 *
 * Order and determinism.  The lists are stable and deterministic, independent of the launch geometry and of the workspace's size.  The
 * compaction is three launches per launch set -- a count per workgroup of 256 items (wave-64 ballots and popcounts, the waves joined
 * in LDS), a scan of the workgroup totals per frame and list, a scatter -- and no workgroup waits for another inside a launch: no
 * look-back, no spin, no grid barrier, no atomic.
 *
 * The call only enqueues on `stream` (a hipStream_t; NULL = the default stream): no host read-back.  It waits for the device only when
 * its workspace has to grow (the first call, or a larger one than before).  ONE stream per ctx at a time.
 *
 * MDVT_ERR_INVALID_ARG, before anything is launched or written: NULL params, opts, io, depth_rgb or counts; point_rgb without
 * color_rgb; with more than one frame a points, point_rgb or used_index stride below a full frame's worth (24 N, 3 N, 4 N bytes), a
 * vertices stride below 24 N, a triangles stride below 24 (H-1)(W-1), a depth or colour stride below H pitches; f64 outputs (and their
 * strides) not 8-byte aligned; i32 and u32 outputs (and their strides) not 4-byte aligned; a frame below 2 x 2; n_frames < 1; a pitch
 * below 3 W; max_depth, a focal length or depth_scale not > 0.
 * MDVT_ERR_UNSUPPORTED, likewise: N > 2^28; decode outside {0, 1}; non-zero reserved; a pose that is not affine.
 *
 * Footprint: per frame 3 N doubles of vertices, the first M triples of triangles, the first U entries of used_index, points and
 * point_rgb, and 2 n_frames words of counts.  Entries beyond a count, up to the stride, are not touched; nothing else of the caller's is
 * written.  The result depends on no byte beyond the first 3 W of an input row.  All pitches, strides and frame offsets are 64-bit.
 * Workspace, from the context's pool under the one growth rule of its scratch blocks: per frame of a launch set 2 (H-1)(W-1) bytes
 * of triangle flags and 4 bytes per 256 triangles and per 256 vertices; bounded by mdvt_config.workspace_mib -- a large batch runs in
 * launch sets. */
int mdvt_export_geometry_batch(mdvt_ctx* ctx, int n_frames, const mdvt_frame_params* params, const mdvt_geometry_opts* opts,
                               const mdvt_geometry_io* io, void* stream);

/* The grey depth of cmf:752-760 for n_frames frames of the context's W x H at d_depth_rgb + k * stride + row * pitch.  The depth is
 * decoded as decode = 0 above (without a depth_scale), then
 *   bits = 16: np.rint(depth * f32(255^2 / max_depth)) as u16, [H][W] at d_out + k * out_stride + row * out_pitch (2 W bytes a row);
 *   bits = 8:  np.rint(depth * f32(255 / max_depth)) as u8, written three times per pixel, [H][W][3] (np.repeat; 3 W bytes a row).
 * Both are one f32 multiply and a rounding half to even.
 * DECREE.  Codes above the encoder's own maximum 255^4 (R << 24 | B << 16 can exceed it) give a value beyond the type's
 * range.  There NumPy's cast is undefined; this call saturates: 65535, 255.  tests/test_geometry_cpu.py holds that no code at or below
 * 255^4 leaves the range.
 * Only enqueues on `stream`; no workspace.
 * MDVT_ERR_INVALID_ARG, before anything is written: NULL d_depth_rgb or d_out, n_frames < 1, bits other than 8 and 16, max_depth
 * not > 0, pitch below 3 W, out_pitch below a row, a stride below H pitches (more than one frame), bits = 16 with d_out, out_pitch or
 * out_stride odd.  MDVT_ERR_UNSUPPORTED: W * H > 2^28.
 * Footprint: the first 2 W (bits = 16) or 3 W (bits = 8) bytes of each of the H rows of each output frame, nothing else of the
 * caller's; the result depends on no byte beyond the first 3 W of an input row.  All pitches and strides are 64-bit. */
int mdvt_depth_grey_batch(mdvt_ctx* ctx, int n_frames, const uint8_t* d_depth_rgb, size_t pitch, size_t stride,
                          double max_depth, int bits, void* d_out, size_t out_pitch, size_t out_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif
