// mdvt_grid_decls.h -- what the rasterising translation units define, declared once per sub-pixel grid: included by
// mdvt_internal.h inside namespace mdvt::grid8 and again inside mdvt::grid4 (no include guard on purpose).  The translation
// units themselves are compiled with -DMDVT_SUBPIX_BITS=8 / 4 and put their definitions into mdvt::MDVT_GRID.
// mdvt_render_dispatch.hip: one launch set through the kernels below, and the LDS sizing rule of the row kernels (at most a CU's 160 KB)
hipError_t launch_render(RenderPlan& plan, const RenderArgs& a, hipStream_t s);
constexpr size_t kMaxLds = 160 * 1024;
size_t render_lds_bytes(const RenderPlan& plan, int W);
bool render_fits_lds(const RenderPlan& plan, int W);      // can the pure-shift row kernels hold a row of this width in LDS?
size_t mesh_rows_tie_bytes(int W);
// mdvt_points_edge_rows.hip: the pure-shift points rows (four pixels a lane; a pixel a lane), the edge points placed after a pure-shift render,
// byte mask -> packed mask and hole counts behind a render that did not produce them, and the fused kernel's conditions
hipError_t launch_points_rows_vec4(RenderPlan& plan, const RenderArgs& a, hipStream_t s);
hipError_t launch_points_rows_px1(const RenderPlan& plan, const RenderArgs& a, hipStream_t s);
hipError_t launch_edge_rows_pure(const RenderPlan& plan, const RenderArgs& a, hipStream_t s);
hipError_t launch_edge_rows_exact(const RenderPlan& plan, const RenderArgs& a, hipStream_t s);
hipError_t launch_pack_mask(const RenderArgs& a, int n, hipStream_t s);
hipError_t launch_reduce_counts(const RenderArgs& a, int n, hipStream_t s);
bool points_fused_bits_applies(const RenderPlan& plan, const RenderArgs& a);      // k_points_rows_fast with the mask compaction fused in (byte masks optional)
hipError_t launch_divcheck(float mult, float scale, float dl, uint32_t* bad, hipStream_t s);      // FrameDev.div_slot: the short division tried on every depth code
// mdvt_general_paths.hip: the general points path and the general mesh path, each whole; the general paths' edge-point splat into the
// global edge keys, and the pass that empties the written words again
hipError_t launch_points_general(const RenderPlan& plan, const RenderArgs& a, hipStream_t s);
hipError_t launch_mesh_general(const RenderPlan& plan, const RenderArgs& a, hipStream_t s);
hipError_t launch_edge_points_splat(const RenderArgs& a, int n, bool as_list, bool counters_zeroed, hipStream_t s);
hipError_t launch_edge_keys_reset(const RenderArgs& a, int n, hipStream_t s);
hipError_t launch_edge_point_pixels(const uint8_t* depth, size_t pitch, const FrameDev* fp, int W, int H, int of_by_one, int how,
                                    int32_t* out, hipStream_t s);
// mdvt_mesh_rows.hip: the pure-shift mesh rows, one workgroup per output row
hipError_t launch_mesh_rows(const RenderPlan& plan, const RenderArgs& a, hipStream_t s);
// mdvt_mesh_band.hip: the pure-shift mesh rows as bands (no edge removal)
bool mesh_band_supported(const RenderPlan& plan, const RenderArgs& a);
hipError_t launch_mesh_band(const RenderPlan& plan, const RenderArgs& a, hipStream_t s);
// mdvt_mesh_band3.hip: the same rows with no vertex records in LDS, both eyes per pass, three workgroups per CU
bool mesh_band3_supported(const RenderPlan& plan, const RenderArgs& a);
hipError_t launch_mesh_band3(const RenderPlan& plan, const RenderArgs& a, hipStream_t s);
// mdvt_mesh_conv.hip: mesh + convergence only, z-buffer in LDS (the product default of movie_2_3D.py:433-445)
bool mesh_conv_supported(const RenderPlan& plan, const RenderArgs& a);
hipError_t launch_mesh_conv(const RenderPlan& plan, const RenderArgs& a, hipStream_t s);
// mdvt_mesh_general.hip: the rasteriser of the general mesh path (between the vertex pass and the resolve pass)
hipError_t launch_mesh_raster_general(const RenderPlan& plan, const RenderArgs& a, hipStream_t s);
// mdvt_msaa.hip: the opt-in 4x multisampled render of n frames (raster into the key planes, then the resolve)
hipError_t launch_msaa_render(const MsaaArgs& a, int n, hipStream_t s);
// mdvt_near_clip.hip: the opt-in near-plane clipping render of n mesh frames with 1 or 4 samples.  flags ([slot][eye], zeroed by the
// caller): detect the eyes where some triangle straddles the plane and re-render only those; nullptr: render every eye
hipError_t launch_near_clip_render(const MsaaArgs& a, int n, int samples, uint32_t* flags, hipStream_t s);
