// mdvt_render_dispatch.hip -- launch_render: which hand-written gfx950 (CDNA4) kernels render one launch set of the stereo-rerender
// hot path, and the LDS sizing rule of the row kernels.  Host code only: no kernel and no tuning hook compiled in (the run-time
// hooks go through tuning_env()), so its two objects, one per sub-pixel grid, go into both libraries unchanged (Makefile).
//
// The kernels replace the Open3D/OpenGL stage of the reference's frame loop (stereo_rerender.py:512-907): decode (dfh:63-75, 13-24)
// -> master scale (sr:541) -> unproject (dmt:1112-1133) -> eye/pose transform (sr:615-619, 724-725, 832-836) -> z-buffered render
// (dmt:1422-1572) -> colour-key hole mask (sr:740, 793) -> edge-point splat (sr:745-814).  They are in mdvt_points_edge_rows.hip
// (points rows; the edge points placed after a pure-shift render), mdvt_general_paths.hip (general points, edge lists, resolve),
// mdvt_mesh_rows.hip (k_mesh_rows) and mdvt_mesh_*.hip.  Everything depends on the sub-pixel grid: one namespace MDVT_GRID, compiled
// once per grid (Makefile).  The kernels that depend on neither are in mdvt_formats.hip, mdvt_edge_filter.hip and mdvt_telea_levels.hip.
//
// The path is an HBM-bound gather/scatter: no MFMA.  What matters is (i) every HBM byte is read and
// written once, coalesced (12 B/lane dwordx3 = 768 contiguous bytes per wave), (ii) the z-buffer
// lives in LDS for the row-local (pure stereo shift) case so the atomics never leave the CU,
// (iii) one launch covers a whole batch of frames (n_frames * H workgroups >> 256 CUs).
#include "mdvt_device.h"

namespace mdvt {
namespace MDVT_GRID {      // one copy per sub-pixel grid (mdvt_internal.h)

// (kMaxLds, a CU's 160 KB: mdvt_grid_decls.h)
bool render_fits_lds(const RenderPlan& plan, int W)
{
    RenderPlan p = plan;
    p.general = 0;
    return render_lds_bytes(p, W) <= kMaxLds;
}

size_t mesh_rows_tie_bytes(int W) { return (((size_t)W + 31) / 32 + 1) * sizeof(uint32_t) + 32; }     // RowTies + alignment slack

size_t render_lds_bytes(const RenderPlan& plan, int W)
{
    if (plan.general) return 0;
    if (plan.mode == MDVT_MODE_POINTS) {
        size_t b = (2 * (size_t)W + 2) * sizeof(u64) + 64;       // + the trash word and the per-wave counters of the fast kernel
        if (plan.edge_points) b += 2 * (size_t)W * sizeof(uint32_t);
        return b;
    }
    const size_t extra = (size_t)W * sizeof(u64) + (plan.edge_points ? (size_t)W * sizeof(uint32_t) + 2 * (size_t)W + 16 : 0) +
                         (plan.remove_edges ? (((size_t)W + 15) & ~(size_t)15) : 0) + mesh_rows_tie_bytes(W);
    size_t b = 2 * (size_t)W * 16 + extra;              // 16-byte vertices (colour in LDS)
    if (b > kMaxLds) b = 2 * (size_t)W * 12 + extra;    // 12-byte vertices (colour re-read in the resolve)
    return b;
}

hipError_t launch_render(RenderPlan& plan, const RenderArgs& a, hipStream_t s)
{
    plan.fused_bits = 0;
    if (plan.mode == MDVT_MODE_POINTS) {
        if (plan.general) return launch_points_general(plan, a, s);
        // (the edge points stay inside k_points_rows: placed afterwards, as for the mesh below, 58.5 k against 61 k frames/s at 1080p)
        const hipError_t e = plan.vec4 ? launch_points_rows_vec4(plan, a, s) : launch_points_rows_px1(plan, a, s);
        return e != hipSuccess ? e : launch_edge_rows_exact(plan, a, s);
    }
    if (plan.conv) return launch_mesh_conv(plan, a, s);
    if (plan.general) return launch_mesh_general(plan, a, s);
    hipError_t e;
    // pure-shift mesh frames: the row kernel renders without edge points, k_edge_rows_pure / k_edge_rows_exact place them afterwards
    // (tuning build: MDVT_EDGE_INBAND=1 keeps them inside the row kernels, as until r04, for the A/B)
    const bool edge_after = plan.remove_edges && plan.edge_points && a.W <= 65535 && tuning_env(TUNE_EDGE_INBAND) == nullptr;
    RenderPlan rp = plan;
    if (edge_after) rp.edge_points = 0;
    // (tuning build: MDVT_MESH_BAND3=0 / 1 picks k_mesh_band / k_mesh_band3 for the A/B)
    const char* b3 = tuning_env(TUNE_MESH_BAND3);
    const bool band3 = b3 ? b3[0] == '1' : false;
    if (band3 && mesh_band3_supported(rp, a) && tuning_env(TUNE_MESH_OLD) == nullptr) e = launch_mesh_band3(rp, a, s);
    else if (mesh_band_supported(rp, a) && tuning_env(TUNE_MESH_OLD) == nullptr) e = launch_mesh_band(rp, a, s);
    else e = launch_mesh_rows(rp, a, s);
    plan.fused_bits = rp.fused_bits;
    if (e == hipSuccess && edge_after) e = launch_edge_rows_pure(plan, a, s);
    return e != hipSuccess ? e : launch_edge_rows_exact(plan, a, s);
}

}  // namespace MDVT_GRID
}  // namespace mdvt
