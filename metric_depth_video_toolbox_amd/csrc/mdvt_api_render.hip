// mdvt_api_render.hip -- the render half of the C ABI of include/mdvt.h: the preparation of frame parameters, the render workspace
// (ensure_workspace; its layout is mdvt_workspace.h), the multisampled and near-clipping renders, mdvt_render_stereo_batch as a list of
// steps, and the entry points beside it that stage frame parameters (mdvt_edge_point_pixels, mdvt_edge_filter) or read the workspace
// (mdvt_debug_read), and the viewer's two calls (include/mdvt_view.h): mdvt_render_view_batch, the batch render with one eye's work,
// and mdvt_view_centers, which stages the parameters and runs the edge filter, and the geometry export's two calls (include/mdvt_geometry.h):
// mdvt_export_geometry_batch, in launch sets on a scratch block of its own, and mdvt_depth_grey_batch.  Host code only; compiled with -ffp-contract=off (the f64 composition of the eye matrices below is part of the
// arithmetic decree).
#include "mdvt_context.h"
#include "mdvt_view.h"
#include "mdvt_geometry.h"

#include <math.h>

#include <algorithm>

using namespace mdvt;
using namespace mdvt::host;
using namespace mdvt::grid8;          // grid-independent launchers of the rasterising translation units; the renders go through MDVT_GRID_CALL

namespace {

constexpr int kWorkspaceChunk = 8;    // frames per launch when a global workspace is needed

// Everything the kernels need about one frame, derived in f64 and rounded once to f32.
// Pure-shift frames: on which row does the chain (mdvt_device.h "edge points") put an edge point of source row i?  Without
// pose and convergence the row is round( ((gy - cy) z / fy sH) (1/z) fyr + cyr ): in exact arithmetic independent of z,
//   v*(i) = (gy_i - cy) sH (fyr / fy) + cyr  ~  i + 1/2 - i / H^2   (mesh grid, cy = H/2),
// a hair below the tie i + 1/2 -- by less than the f32 rounding of fy (dmt:1058) moves it for the first rows, which then land
// on i + 1 -- and the eight f64 roundings of the chain move v by at most 8 H 2^-53.  Rows whose v* keeps a margin of four
// times that from a tie have their row decided here, once per camera matrix; the others (a tie in exact arithmetic: the
// roundings of each point decide) and the rows that land on i + 1 form [erow_lo, erow_hi), left to k_edge_rows_exact.
static void edge_row_range(FrameDev& f, int H)
{
    const long double fy = f.Kd[1], cy = f.Kd[3], sH = f.sHd, fyr = (long double)f.fyr, cyr = (long double)f.cyr;
    const long double margin = 32.0L * 1.1102230246251565e-16L * ((long double)H + fabsl(cyr) + 1.0L);
    int lo = H, hi = 0;
    bool wild = false;
    for (int i = 0; i < H; ++i) {
        const long double gy = f.sy == 1.0f ? (long double)i : (long double)((float)i * f.sy);
        const long double v = (gy - cy) * sH * (fyr / fy) + cyr;
        const long double fl = floorl(v);
        const bool undecided = fabsl(v - (fl + 0.5L)) <= margin;
        const long double row = undecided ? fl : floorl(v + 0.5L);           // undecided: fl or fl + 1
        const bool plain = !undecided && row == (long double)i;
        if (plain) continue;
        if (row != (long double)i && !(!undecided && row == (long double)i + 1.0L)) { wild = true; break; }
        if (i < lo) lo = i;
        if (i + 1 > hi) hi = i + 1;
    }
    f.erow_wild = wild ? 1 : 0;
    f.erow_lo = (wild || lo >= hi) ? 0 : lo;
    f.erow_hi = (wild || lo >= hi) ? 0 : hi;
}

int fill_frame_dev(mdvt_ctx* c, const mdvt_frame_params& p, FrameDev& f)
{
    const mdvt_config& cfg = c->cfg;
    const int W = c->W, H = c->H;
    const double fx = p.K[0], fy = p.K[4], cx = p.K[2], cy = p.K[5];
    const double fxr = p.Krender[0], fyr = p.Krender[4], cxr = p.Krender[2], cyr = p.Krender[5];
    if (!(fx > 0.0) || !(fy > 0.0) || !(fxr > 0.0) || !(fyr > 0.0))
        return fail(c, MDVT_ERR_INVALID_ARG, "camera matrix needs positive focal lengths");
    if (cxr * 2.0 != (double)W || cyr * 2.0 != (double)H)
        return fail(c, MDVT_ERR_UNSUPPORTED,
                    "render size (2*cx, 2*cy) = (%g, %g) differs from the frame size %dx%d (--vr180 is not built)",
                    cxr * 2.0, cyr * 2.0, W, H);
    if (!(p.depth_scale > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "depth_scale must be > 0");
    memset(&f, 0, sizeof f);
    f.mult = (float)(cfg.max_depth / 4228250625.0);
    f.scale = (float)p.depth_scale;
    const double half = cfg.ipd_m / 2.0;
    f.dl = (float)(fxr * half);
    f.fx = (float)fx; f.fy = (float)fy; f.cx = (float)cx; f.cy = (float)cy;
    f.fxr = (float)fxr; f.fyr = (float)fyr; f.cxr = (float)cxr; f.cyr = (float)cyr;
    const bool mesh = cfg.mode == MDVT_MODE_MESH;
    f.sx = mesh ? (float)(((double)W + 1.0) / (double)W) : 1.0f;
    f.sy = mesh ? (float)(((double)H + 1.0) / (double)H) : 1.0f;
    f.sW = (float)(((double)W - 1.0) / (double)W);
    f.sH = (float)(((double)H - 1.0) / (double)H);
    f.Kd[0] = fx; f.Kd[1] = fy; f.Kd[2] = cx; f.Kd[3] = cy;
    f.rKd[0] = 1.0 / fx; f.rKd[1] = 1.0 / fy;
    const double conv = (p.convergence_angle == p.convergence_angle) ? p.convergence_angle : 0.0;   // NaN -> none
    const bool same_k = fx == fxr && fy == fyr && cx == cxr && cy == cyr;
    f.general = (p.has_T || conv != 0.0 || !same_k) ? 1 : 0;
    double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (p.has_T) {
        memcpy(T, p.T, sizeof T);
        if (fabs(T[12]) > 1e-12 || fabs(T[13]) > 1e-12 || fabs(T[14]) > 1e-12 || fabs(T[15] - 1.0) > 1e-12)
            return fail(c, MDVT_ERR_UNSUPPORTED, "pose matrix must be affine (last row 0 0 0 1)");
    }
    for (int eye = 0; eye < 2; ++eye) {
        // M = Translate(+-ipd/2) * Ry(-+a) * T;  Ry(t) = [[c,0,s],[0,1,0],[-s,0,c]]
        const double t = eye == 0 ? -conv : conv;
        const double cs = cos(t), sn = sin(t);
        const double R[3][3] = {{cs, 0.0, sn}, {0.0, 1.0, 0.0}, {-sn, 0.0, cs}};
        const double shift[3] = {eye == 0 ? half : -half, 0.0, 0.0};
        for (int r = 0; r < 3; ++r) {
            for (int col = 0; col < 3; ++col)
                f.M[eye][4 * r + col] = (float)((R[r][0] * T[0 + col] + R[r][1] * T[4 + col]) + R[r][2] * T[8 + col]);
            f.M[eye][4 * r + 3] = (float)(((R[r][0] * T[3] + R[r][1] * T[7]) + R[r][2] * T[11]) + shift[r]);
        }
    }
    // The edge points' chain takes the reference's operands as they are (mdvt_device.h "edge points")
    f.sWd = ((double)W - 1.0) / (double)W;
    f.sHd = ((double)H - 1.0) / (double)H;
    f.hd = half;
    f.has_T = p.has_T ? 1 : 0;
    memcpy(f.Td, T, sizeof T);
    f.has_conv = conv != 0.0 ? 1 : 0;
    f.cs[0] = cos(conv); f.cs[1] = sin(conv);
    if (!f.general && cfg.remove_edges && cfg.edge_points) {
        const double key[5] = {f.Kd[1], f.Kd[3], (double)f.fyr, (double)f.cyr, (double)f.sy};
        if (!(c->erow_cached && memcmp(key, c->erow_key, sizeof key) == 0)) {
            edge_row_range(f, H);
            memcpy(c->erow_key, key, sizeof key);
            c->erow_val[0] = f.erow_lo; c->erow_val[1] = f.erow_hi; c->erow_val[2] = f.erow_wild;
            c->erow_cached = true;
        }
        f.erow_lo = c->erow_val[0]; f.erow_hi = c->erow_val[1]; f.erow_wild = c->erow_val[2];
    }
    // Convergence and nothing else (sr:707-726: rotation about the camera's y axis, shift along x): the projected row of a
    // vertex is depth independent, v = (gy - cy) / rz(j) + cy with rz(j) = m10 + m8 (gx_j - cx) / fx, which k_mesh_conv
    // (mdvt_mesh_conv.hip) builds on.  It takes the frame if the vertex rows stay low staircases: at most 12 rows of tilt
    // across the frame (its row tags are 5 bits, its column pairs expect neighbouring brackets to differ by one).
    f.conv_band = 0;
    if (mesh && !p.has_T && conv != 0.0 && same_k) {
        bool ok = true;
        for (int eye = 0; eye < 2 && ok; ++eye) {
            const float* M = f.M[eye];
            ok = M[1] == 0.0f && M[4] == 0.0f && M[5] == 1.0f && M[6] == 0.0f && M[7] == 0.0f && M[9] == 0.0f && M[11] == 0.0f;
            const double rz0 = (double)M[10] + (double)M[8] * ((0.0 - cx) / fx);
            const double rz1 = (double)M[10] + (double)M[8] * (((double)(W - 1) * ((double)W + 1.0) / (double)W - cx) / fx);
            if (!(rz0 > 0.5 && rz1 > 0.5 && rz0 < 2.0 && rz1 < 2.0)) ok = false;
            else if (fabs(1.0 / rz0 - 1.0 / rz1) * ((double)H * 0.5 + 1.0) * (fyr / fy) > 12.0) ok = false;
        }
        f.conv_band = ok ? 1 : 0;
    }
    return MDVT_OK;
}

// Stage n FrameDev records to the device through the pinned ring; returns the device pointer.
int stage_params(mdvt_ctx* c, const std::vector<FrameDev>& v, hipStream_t s, const FrameDev** dev, ParamSlot** slot_out)
{
    if (c->last_slot && c->last_stream == s && c->last_staged.size() == v.size() &&
        memcmp(c->last_staged.data(), v.data(), v.size() * sizeof(FrameDev)) == 0) {
        // identical to what already sits on the device (stream order keeps the earlier copy ahead of us)
        *dev = c->last_slot->dev;
        *slot_out = c->last_slot;
        return MDVT_OK;
    }
    ParamSlot& sl = c->slots[c->next_slot];
    c->next_slot = (c->next_slot + 1) % kParamSlots;
    if (sl.used) MDVT_HIP(c, hipEventSynchronize(sl.done));     // slot is being reused: its last user must be done
    if (sl.capacity < v.size()) {
        pool_give(sl.host, sl.dev, sl.capacity * sizeof(FrameDev), c->pool_tag);
        sl.host = nullptr; sl.dev = nullptr; sl.capacity = 0;
        size_t cap = 16;
        while (cap < v.size()) cap *= 2;
        void *h = nullptr, *d = nullptr;
        size_t got = 0;
        MDVT_HIP(c, pool_take(cap * sizeof(FrameDev), true, c->pool_tag, &h, &d, &got));
        sl.host = (FrameDev*)h; sl.dev = (FrameDev*)d; sl.capacity = got / sizeof(FrameDev);
    }
    if (!sl.done) MDVT_HIP(c, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    memcpy(sl.host, v.data(), v.size() * sizeof(FrameDev));
    MDVT_HIP(c, hipMemcpyAsync(sl.dev, sl.host, v.size() * sizeof(FrameDev), hipMemcpyHostToDevice, s));
    sl.used = true;
    c->last_staged = v;
    c->last_slot = &sl;
    c->last_stream = s;
    *dev = sl.dev;
    *slot_out = &sl;
    return MDVT_OK;
}

RenderWorkspaceLayout layout_of(const mdvt_ctx* c) { return RenderWorkspaceLayout(c->W, c->H, c->ws_frames, c->huge_lists); }
// (the EMPTY fill of fresh key buffers goes on the caller's stream: PyTorch's pool streams do not synchronise with the
//  legacy null stream, so a fill issued there could land after the first splat)
// (eyes: 1 for a view render, which needs eye 0's planes only; a context that has rendered nothing but views holds no plane of a
//  second eye, and its first stereo render replaces the workspace as a larger launch set would)
int ensure_workspace(mdvt_ctx* c, int frames, bool need_keys, bool need_ekeys, bool need_edges, bool need_mesh_ws, hipStream_t s, int eyes = 2)
{
    const bool grow = frames > c->ws_frames || eyes > c->ws_eyes;
    // (blocks that are replaced go back to the pool, where another context may pick them up at once: whatever was submitted
    //  with them -- to any stream -- has to be through first; hipFree used to wait for that implicitly)
    if (grow && c->ws_bytes) MDVT_HIP(c, hipDeviceSynchronize());
    // (not growing, yet a group that is not complete holds a buffer: an earlier call failed half-way through allocating it -- its
    //  asynchronous fill may still be pending, and the block must not reach the pool before that is through)
    if (!grow && ((need_keys && !c->ws_keys && (c->keys[0] || c->keys[1])) || (need_ekeys && !c->ws_ekeys && (c->ekeys[0] || c->ekeys[1] || c->elist)) ||
                  (need_edges && !c->ws_edges && (c->tri_invalid || c->unused)) || (need_mesh_ws && !c->ws_mesh && (c->cbuf[0] || c->cbuf[1]))))
        MDVT_HIP(c, hipDeviceSynchronize());
    auto drop = [c](auto*& p) { ws_free(c, p); p = nullptr; };      // (ws_free takes a null pointer)
    if (grow || (need_keys && !c->ws_keys)) { drop(c->keys[0]); drop(c->keys[1]); c->ws_keys = false; }
    if (grow || (need_ekeys && !c->ws_ekeys)) { drop(c->ekeys[0]); drop(c->ekeys[1]); drop(c->elist); c->ws_ekeys = false; }
    if (grow || (need_edges && !c->ws_edges)) { drop(c->tri_invalid); drop(c->unused); c->ws_edges = false; }
    if (grow || (need_mesh_ws && !c->ws_mesh)) { drop(c->cbuf[0]); drop(c->cbuf[1]); c->ws_mesh = false; }
    if (grow) { c->ws_frames = std::max(frames, c->ws_frames); c->ws_eyes = std::max(eyes, c->ws_eyes); }
    // (tuning build, the r04 diagnosis: MDVT_WS_LAYOUT=joint puts the second bank's huge list back into the queue block, as at 47b4117 --
    //  2.2 MB for a 100 x 31 frame; it takes effect when that block is made, so it is read before the layout is)
    if (need_mesh_ws && !c->ws_mesh) { const char* e = tuning_env(TUNE_WS_LAYOUT); c->huge_lists = (e && strcmp(e, "joint") == 0) ? 2 : 1; }
    const RenderWorkspaceLayout L = layout_of(c);
    if (need_keys && !c->ws_keys) {
        for (int e = 0; e < c->ws_eyes; ++e) {
            MDVT_HIP(c, ws_malloc(c, (void**)&c->keys[e], L.plane_bytes(), s));
            MDVT_HIP(c, hipMemsetAsync(c->keys[e], 0xFF, L.plane_bytes(), s));     // parity 0's empty value
        }
        c->key_parity = 0;
        c->ws_keys = true;
    }
    if (need_ekeys && !c->ws_ekeys) {
        for (int e = 0; e < c->ws_eyes; ++e) {
            MDVT_HIP(c, ws_malloc(c, (void**)&c->ekeys[e], L.plane_bytes(), s));
            MDVT_HIP(c, hipMemsetAsync(c->ekeys[e], 0xFF, L.plane_bytes(), s));
        }
        MDVT_HIP(c, ws_malloc(c, (void**)&c->elist, L.elist_bytes(), s));
        MDVT_HIP(c, hipMemsetAsync(c->elist + L.elist_count_at(), 0, L.slots * L.H * sizeof(uint32_t), s));   // counters; the reset pass keeps them 0
        c->ws_ekeys = true;
    }
    if (need_mesh_ws && !c->ws_mesh) {
        for (int e = 0; e < c->ws_eyes; ++e) MDVT_HIP(c, ws_malloc(c, (void**)&c->cbuf[e], L.plane_bytes(), s));   // tie side words: a word is initialised by the fragment that marks its pixel, so the plane needs no clearing
        drop(c->bigq);
        // (entry indices are 32-bit: chunk_of() keeps a launch set's slots * npx * 4 below 2^32)
        if (queue_slots_max(c->W, c->H) < 1) return fail(c, MDVT_ERR_UNSUPPORTED, "general mesh path: a %d x %d frame exceeds the 32-bit triangle queue", c->W, c->H);
        size_t pad = 0;      // (tuning build: MDVT_WS_PAD=n appends n unused bytes to the queue block)
        if (const char* e = tuning_env(TUNE_WS_PAD)) pad = (size_t)strtoull(e, nullptr, 10);
        c->bigq_bytes = L.queue_bytes(); c->bigq_counters_at = L.counters_at();
        MDVT_HIP(c, ws_malloc(c, (void**)&c->bigq, c->bigq_bytes + pad, s));
        c->ws_mesh = true;
    }
    if (need_edges && !c->ws_edges) {
        MDVT_HIP(c, ws_malloc(c, (void**)&c->tri_invalid, L.tri_invalid_bytes(), s));
        MDVT_HIP(c, ws_malloc(c, (void**)&c->unused, L.unused_bytes(), s));
        c->ws_edges = true;
    }
    return MDVT_OK;
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

// The decree's snap (mdvt_device.h) on the host: same IEEE operations (this file is compiled with -ffp-contract=off).
int host_snap(float x, int subpix)
{
    x = fminf(fmaxf(x, -kSnapLimit), kSnapLimit);
    return (int)rintf(x * (float)subpix);
}

// Scanline k (centre S k + S/2) is covered by the cell row c = largest i with snap(f32(i) * sy) < centre (a centre ON a vertex
// row belongs to the cells above it: bottom edges own their centres, mdvt_device.h edge_in), if that is not the last vertex
// row (k_mesh_rows derives the same per workgroup).
int ensure_rowcell(mdvt_ctx* c, hipStream_t s)
{
    if (c->rowcell && c->rowcell_bits == grid_bits(c)) return MDVT_OK;
    const int H = c->H;
    const int kSubpix = 1 << grid_bits(c);        // (shadows the compile-time grid of this translation unit on purpose)
    const float sy = (float)(((double)H + 1.0) / (double)H);
    std::vector<mdvt::RowCell> t((size_t)H);
    for (int k = 0; k < H; ++k) {
        const int Yc = k * kSubpix + kSubpix / 2;
        int ilo = (int)(((float)k + 0.5f) / sy);
        ilo = ilo < 0 ? 0 : (ilo > H - 1 ? H - 1 : ilo);
        while (ilo > 0 && host_snap((float)ilo * sy, kSubpix) >= Yc) --ilo;
        while (ilo + 1 <= H - 1 && host_snap((float)(ilo + 1) * sy, kSubpix) < Yc) ++ilo;
        mdvt::RowCell r{};
        r.c = (ilo <= H - 2) ? ilo : -1;
        r.Yt = r.c >= 0 ? host_snap((float)r.c * sy, kSubpix) : 0;
        r.Yb = r.c >= 0 ? host_snap((float)(r.c + 1) * sy, kSubpix) : 1;
        t[(size_t)k] = r;
    }
    if (!c->rowcell) MDVT_HIP(c, ws_malloc(c, (void**)&c->rowcell, (size_t)H * sizeof(mdvt::RowCell), s));
    else MDVT_HIP(c, hipDeviceSynchronize());     // a render of the other grid may still read the table
    c->rowcell_bits = grid_bits(c);
    MDVT_HIP(c, hipMemcpyAsync(c->rowcell, t.data(), (size_t)H * sizeof(mdvt::RowCell), hipMemcpyHostToDevice, s));
    MDVT_HIP(c, hipStreamSynchronize(s));      // `t` is pageable host memory
    return MDVT_OK;
}

// What RenderArgs and MsaaArgs share: the caller's images, the staged parameters, the frame size and the slot strides.
template <class Args>
void bind_io(Args& a, const mdvt_ctx* c, const mdvt_io* io, const FrameDev* dfp)
{
    a.depth = io->depth_rgb; a.depth_pitch = io->depth_pitch; a.depth_stride = io->depth_stride;
    a.color = io->color_rgb; a.color_pitch = io->color_pitch; a.color_stride = io->color_stride;
    a.rgb[0] = io->left_rgb; a.rgb[1] = io->right_rgb; a.rgb_pitch = io->rgb_pitch; a.rgb_stride = io->rgb_stride;
    a.mask[0] = io->left_mask; a.mask[1] = io->right_mask; a.mask_pitch = io->mask_pitch; a.mask_stride = io->mask_stride;
    a.hole_counts = io->hole_counts; a.fp = dfp; a.key_rgb = packed_key_rgb(c);
    a.W = c->W; a.H = c->H; a.ws_stride_px = (size_t)c->W * c->H; a.ws_stride_tri = 2 * (size_t)(c->W - 1) * (c->H - 1);
}

// The edge filter's flags of the n frames from a.frame0 on, into the workspace slots that tri_invalid / unused start at.
template <class Args>
int filter_edges(mdvt_ctx* c, const Args& a, int n, uint8_t* tri_invalid, uint8_t* unused, hipStream_t s)
{
    MDVT_HIP(c, launch_zero_bytes(unused, (size_t)n * a.ws_stride_px, s));
    MDVT_HIP(c, launch_edge_filter(a.depth, a.depth_pitch, a.depth_stride, a.fp, a.frame0, n, a.W, a.H, c->cfg.mode == MDVT_MODE_MESH,
                                   tri_invalid, a.ws_stride_tri, unused, a.ws_stride_px, s));
    return MDVT_OK;
}

// ---- 4x multisampled render (mdvt_config.samples = 4; mdvt_msaa.hip) ---------------------------------------------------------
// What the mode does not cover is refused before anything is checked or launched, with the output named.
int msaa_refusal(mdvt_ctx* c, const mdvt_io* io, const char* mode = "multisampling (samples = 4)")
{
    const char* what = nullptr;
    if (c->cfg.edge_points) what = "edge points (mdvt_config.edge_points != 0)";
    else if (io->left_depth || io->right_depth) what = "depth planes (left_depth / right_depth)";
    else if (io->left_seed || io->right_seed) what = "seed images (left_seed / right_seed)";
    else if (io->left_maskbits || io->right_maskbits) what = "packed mask bits (left_maskbits / right_maskbits)";
    else if (!io->left_mask || !io->right_mask) what = "a NULL byte mask (left_mask / right_mask are required)";
    if (!what) return MDVT_OK;
    return fail(c, MDVT_ERR_UNSUPPORTED, "%s does not cover %s", mode, what);
}

// Launch sets of up to 16 frames, as many as workspace_mib affords (64 B/px of sample keys, 3 B/px of edge-filter flags).
int render_msaa(mdvt_ctx* c, int n_frames, const std::vector<FrameDev>& fd, const mdvt_io* io, hipStream_t s)
{
    const int W = c->W, H = c->H;
    const size_t npx = (size_t)W * (size_t)H;
    if (2 * npx >= (size_t)0xFFFFFFFFu)
        return fail(c, MDVT_ERR_UNSUPPORTED, "multisampling: a %d x %d frame has more triangles than its 32-bit draw ids can name", W, H);
    const bool rm = c->cfg.remove_edges != 0;
    int chunk = slots_afforded(c, npx * (2 * 4 * sizeof(unsigned long long) + (rm ? kNominalEdgeFlagBytesPerPx : 0)), 16);
    if (chunk > n_frames) chunk = n_frames;

    const FrameDev* dfp = nullptr;
    ParamSlot* slot = nullptr;
    int rc = stage_params(c, fd, s, &dfp, &slot);
    if (rc != MDVT_OK) return rc;
    if (rm && (rc = ensure_workspace(c, chunk, false, false, true, false, s)) != MDVT_OK) return rc;
    const bool clip = c->near_clip && c->cfg.mode == MDVT_MODE_MESH;      // (the clipping render of every frame, mdvt_near_clip.hip)
    const size_t plane_bytes = npx * 2 * 4 * sizeof(unsigned long long);       // one slot, both eyes
    Scratch& keys = c->scratch[SCR_MSAA_KEYS];
    MDVT_HIP(c, scratch_reserve(c, keys, (size_t)chunk * plane_bytes, s, &c->msaa_dirty));
    if (c->msaa_dirty) MDVT_HIP(c, hipMemsetAsync(keys.p, 0xFF, keys.bytes, s));
    c->msaa_dirty = false;
    if (io->hole_counts) MDVT_HIP(c, hipMemsetAsync(io->hole_counts, 0, 2 * (size_t)n_frames * sizeof(uint32_t), s));

    MsaaArgs a{};
    bind_io(a, c, io, dfp);
    a.keys = keys.as<unsigned long long>();
    a.tri_invalid = rm ? c->tri_invalid : nullptr; a.unused = rm ? c->unused : nullptr;
    a.mode = c->cfg.mode; a.cull = c->cfg.cull; a.pattern = c->cfg.sample_pattern; a.resolve = c->cfg.sample_resolve;
    for (int f0 = 0; f0 < n_frames; f0 += chunk) {
        const int n = n_frames - f0 < chunk ? n_frames - f0 : chunk;
        a.frame0 = f0;
        if (rm && (rc = filter_edges(c, a, n, c->tri_invalid, c->unused, s)) != MDVT_OK) return rc;
        c->msaa_dirty = true;
        if (clip) MDVT_HIP(c, MDVT_GRID_CALL(c, launch_near_clip_render, a, n, 4, nullptr, s));
        else MDVT_HIP(c, MDVT_GRID_CALL(c, launch_msaa_render, a, n, s));
        c->msaa_dirty = false;
    }
    MDVT_HIP(c, hipEventRecord(slot->done, s));
    return MDVT_OK;
}

// ---- near-plane clipping, single sample (mdvt_set_near_clip; mdvt_near_clip.hip) -------------------------------------------------
// Runs after the single-sample kernels have rendered every frame of the batch, on the same stream: a detect kernel flags the (frame,
// eye) where some triangle may straddle the plane, and the key-plane kernels re-render only those eyes (the others leave at once;
// nothing is read back).  Launch sets of up to 16 frames, as many as workspace_mib affords (16 B/px of keys; with remove_edges the
// edge filter's flags of the slots the render before has already allocated).
int render_near_clip_gate(mdvt_ctx* c, int n_frames, const FrameDev* dfp, const mdvt_io* io, hipStream_t s)
{
    const int W = c->W, H = c->H;
    const size_t npx = (size_t)W * (size_t)H;
    const bool rm = c->cfg.remove_edges != 0;
    const size_t per_slot = npx * 2 * sizeof(unsigned long long);
    int chunk = slots_afforded(c, per_slot, 16);
    if (rm && chunk > c->ws_frames) chunk = c->ws_frames;        // (the render before has made at least one slot of edge flags)
    if (chunk > n_frames) chunk = n_frames;
    if (chunk < 1) return fail(c, MDVT_ERR_INVALID_ARG, "near-plane clipping: no workspace slot for the edge filter");
    Scratch& keys = c->scratch[SCR_CLIP_KEYS];
    MDVT_HIP(c, scratch_reserve(c, keys, (size_t)chunk * per_slot, s, &c->clip_dirty));
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_CLIP_FLAGS], (size_t)chunk * 2 * sizeof(uint32_t), s));
    uint32_t* const flags = c->scratch[SCR_CLIP_FLAGS].as<uint32_t>();
    if (c->clip_dirty) MDVT_HIP(c, hipMemsetAsync(keys.p, 0xFF, keys.bytes, s));      // (the whole plane, whatever this call uses of it)
    c->clip_dirty = false;

    MsaaArgs a{};
    bind_io(a, c, io, dfp);
    a.keys = keys.as<unsigned long long>();
    a.tri_invalid = rm ? c->tri_invalid : nullptr; a.unused = rm ? c->unused : nullptr;
    a.mode = c->cfg.mode; a.cull = c->cfg.cull;
    for (int f0 = 0; f0 < n_frames; f0 += chunk) {
        const int n = n_frames - f0 < chunk ? n_frames - f0 : chunk;
        a.frame0 = f0;
        MDVT_HIP(c, hipMemsetAsync(flags, 0, (size_t)n * 2 * sizeof(uint32_t), s));
        if (rm) { if (int rc = filter_edges(c, a, n, c->tri_invalid, c->unused, s)) return rc; }      // (mesh mode: near_clip)
        c->clip_dirty = true;
        MDVT_HIP(c, MDVT_GRID_CALL(c, launch_near_clip_render, a, n, 1, flags, s));
        c->clip_dirty = false;
    }
    return MDVT_OK;
}

}  // namespace

extern "C" {

// ---- The steps of mdvt_render_stereo_batch, in its order ---------------------------------------------------------------------
struct BatchFlags { bool no_byte_mask, zout, want_bits, near_clip; };

// Everything that is refused before the device is touched.
static int validate_batch(mdvt_ctx* c, int n_frames, const mdvt_frame_params* params, const mdvt_io* io, BatchFlags& f)
{
    if (n_frames <= 0 || !params || !io) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames/params/io invalid");
    if (!io->depth_rgb || !io->color_rgb || !io->left_rgb || !io->right_rgb)
        return fail(c, MDVT_ERR_INVALID_ARG, "depth_rgb, color_rgb and left/right rgb buffers are required");
    if (c->cfg.samples == 4) { if (int rc = msaa_refusal(c, io)) return rc; }
    f.near_clip = c->near_clip && c->cfg.mode == MDVT_MODE_MESH;     // (points: a GL drops a point behind the plane, as the decree does)
    if (f.near_clip) {
        if (int rc = msaa_refusal(c, io, "near-plane clipping (near_clip = 1)")) return rc;
        // fan triangle f of source triangle d is drawn as 2 d + f: 4 (W - 1) (H - 1) ids in the 32 bits of a key
        if (c->W >= 2 && c->H >= 2 && 4 * (uint64_t)(c->W - 1) * (uint64_t)(c->H - 1) >= (uint64_t)0xFFFFFFFFu)
            return fail(c, MDVT_ERR_UNSUPPORTED, "near-plane clipping: a %d x %d frame has more fan triangles than its 32-bit draw ids can name", c->W, c->H);
    }
    // The byte masks may be left out (both NULL) by a caller that takes the packed mask instead -- where the compaction is fused
    // into the render kernel (pure-shift point frames: checked per launch set in submit_run); everywhere else they are required.
    f.no_byte_mask = !io->left_mask && !io->right_mask && io->left_maskbits && io->right_maskbits;
    if (!f.no_byte_mask && (!io->left_mask || !io->right_mask))
        return fail(c, MDVT_ERR_INVALID_ARG, "left/right mask buffers are required (both may be NULL only when maskbits are given)");
    const int W = c->W, H = c->H;
    if (W < 2 || H < 2) return fail(c, MDVT_ERR_INVALID_ARG, "rendering needs at least a 2x2 frame");
    if (io->depth_pitch < (size_t)3 * W || io->color_pitch < (size_t)3 * W || io->rgb_pitch < (size_t)3 * W ||
        (!f.no_byte_mask && io->mask_pitch < (size_t)W))
        return fail(c, MDVT_ERR_INVALID_ARG, "a pitch is smaller than one row");   // sr:507 shape assert
    f.zout = io->left_depth || io->right_depth;
    if (f.zout && io->zout_pitch < (size_t)4 * W) return fail(c, MDVT_ERR_INVALID_ARG, "zout_pitch smaller than one row");
    if (io->left_seed || io->right_seed) {
        if (!io->left_seed || !io->right_seed) return fail(c, MDVT_ERR_INVALID_ARG, "seed images need both eyes");
        if (!c->cfg.remove_edges) return fail(c, MDVT_ERR_INVALID_ARG, "seed images need remove_edges (the infill-mask mode of sr:568-570)");
        if (io->seed_pitch < (size_t)3 * W) return fail(c, MDVT_ERR_INVALID_ARG, "seed_pitch smaller than one row");
    }
    f.want_bits = io->left_maskbits || io->right_maskbits;
    if (f.want_bits) {
        if (!io->left_maskbits || !io->right_maskbits) return fail(c, MDVT_ERR_INVALID_ARG, "maskbits need both eyes");
        if (io->maskbits_pitch < (size_t)4 * (((size_t)W + 31) / 32) || io->maskbits_pitch % 4 != 0 || io->maskbits_stride % 4 != 0 ||
            ((uintptr_t)io->left_maskbits % 4) || ((uintptr_t)io->right_maskbits % 4))
            return fail(c, MDVT_ERR_INVALID_ARG, "maskbits rows must be dword aligned and at least 4*ceil(W/32) bytes");
    }
    return MDVT_OK;
}

// Pure-shift point frames: the disparity's division proven short per parameter set (FrameDev.div_slot).  A new set costs one
// launch of 65536 threads on this stream, once per context; clips have one set, or one per distinct field of view.
// The checks run on the stream of the call that brought their set in; a call on another stream (a pure-shift point render
// without hole counts uses no other workspace, so nothing else orders it after that call) first waits for the latest check,
// and with it for every earlier one and the table's fill: each check is recorded after a wait for the one before it, whichever
// stream that was on.
static int assign_div_slots(mdvt_ctx* c, std::vector<FrameDev>& fd, hipStream_t s)
{
    bool ordered = false;
    for (FrameDev& f : fd) {
        if (f.general) continue;
        if (!ordered && c->div_done && c->div_stream != s) MDVT_HIP(c, hipStreamWaitEvent(s, c->div_done, 0));
        ordered = true;
        std::array<uint32_t, 3> key;
        memcpy(&key[0], &f.mult, 4); memcpy(&key[1], &f.scale, 4); memcpy(&key[2], &f.dl, 4);
        int slot = -1;
        for (size_t q = c->div_keys.size(); q-- > 0;) if (c->div_keys[q] == key) { slot = (int)q; break; }
        if (slot < 0 && c->div_keys.size() < (size_t)mdvt::kDivSlots) {
            if (!c->divcheck) {
                MDVT_HIP(c, ws_malloc(c, (void**)&c->divcheck, mdvt::kDivSlots * sizeof(uint32_t), s));
                MDVT_HIP(c, hipMemsetAsync(c->divcheck, 0, mdvt::kDivSlots * sizeof(uint32_t), s));
            }
            if (!c->div_done) MDVT_HIP(c, hipEventCreateWithFlags(&c->div_done, hipEventDisableTiming));
            slot = (int)c->div_keys.size();
            MDVT_HIP(c, MDVT_GRID_CALL(c, launch_divcheck, f.mult, f.scale, f.dl, c->divcheck + slot, s));
            MDVT_HIP(c, hipEventRecord(c->div_done, s));
            c->div_stream = s;
            c->div_keys.push_back(key);
        }
        f.div_slot = slot;
    }
    return MDVT_OK;
}

// The arithmetic of a frame (pure shift or general) is its own property, never its batch
// neighbours': consecutive frames of one kind form a run, every run gets its own launches.
struct Run { int f0, f1, general, conv, craster; };  // general = "takes the global-key kernels"; conv = k_mesh_conv (mesh, convergence only);
                                                     // craster = general, but every frame convergence-only: k_mesh_raster_conv
static void build_runs(const mdvt_ctx* c, const RenderPlan& plan, const std::vector<FrameDev>& fd, std::vector<Run>& runs)
{
    const int W = c->W, H = c->H;
    // A pure-shift frame wider than the LDS row kernels can hold (10 240 px for points, ~4 300 for the mesh with edge
    // points) is rendered by the global-key kernels instead -- with its own pure-shift arithmetic (FrameDev.general
    // stays 0), so the pixels do not depend on which kernels ran.  MDVT_FORCE_GLOBAL=1 sends every frame that way (tests).
    const bool wide = !MDVT_GRID_CALL(c, render_fits_lds, plan, W) || tuning_env(TUNE_FORCE_GLOBAL) != nullptr;
    bool conv_kernel = false;
    if (plan.mode == MDVT_MODE_MESH && !wide) {
        RenderArgs probe{};
        probe.W = W; probe.H = H;
        conv_kernel = MDVT_GRID_CALL(c, mesh_conv_supported, plan, probe);
    }
    for (int k = 0; k < (int)fd.size(); ++k) {
        const int cv = (conv_kernel && fd[(size_t)k].conv_band) ? 1 : 0;
        const int g = (!cv && (wide || fd[(size_t)k].general || fd[(size_t)k].erow_wild)) ? 1 : 0;
        const int cr = (g && !wide && plan.mode == MDVT_MODE_MESH && fd[(size_t)k].conv_band) ? 1 : 0;
        if (runs.empty() || runs.back().general != g || runs.back().conv != cv || runs.back().craster != cr) runs.push_back({k, k + 1, g, cv, cr});
        else runs.back().f1 = k + 1;
    }
}

// frames per launch set.  Point splat, general: two frames keep the 64-bit key buffers (33 MB per 1080p frame)
// inside the 256 MiB Infinity Cache between splat and resolve (measured +12 %); the mesh needs the slack of
// eight (rows full of slivers leave a long tail), and the edge filter alone streams, so 8 as well.
static int chunk_of(const mdvt_ctx* c, const RenderPlan& plan, const Run& r, int tuned_chunk)
{
    const int n = r.f1 - r.f0;
    if (!(r.general || plan.remove_edges || (r.conv && plan.edge_points))) return n;                  // no workspace: the whole run in one launch
    // (points, general path: four slots -- one launch set of four frames, or banks of two (submit_run); two slots until r04:
    //  1080p convergence 26.7 k -> 28.2 k frames/s, 4K pose + contention 5.4 k -> 6.1 k)
    int ws_chunk = (r.general && plan.mode == MDVT_MODE_POINTS) ? 4 : kWorkspaceChunk;
    if (r.general && plan.mode == MDVT_MODE_MESH) {
        ws_chunk = 2 * kWorkspaceChunk;      // 16: measured -4 % (convergence) / -11 % (pose) vs 8
        // ~64 B/px per slot (z keys, tie side words, triangle queue; until r04 also 32 B/px of vertex records): 2.1 GB at 1080p,
        // 8.5 GB at 4K; the queue's entry indices are 32-bit, so very large frames get fewer slots (4 entries per pixel and slot)
        const size_t fit = queue_slots_max(c->W, c->H);
        if ((size_t)ws_chunk > fit) ws_chunk = fit < 1 ? 1 : (int)fit;
        // ... and the slots have to fit the context's workspace budget (mdvt_config.workspace_mib, default 4 GiB: 16 slots at
        // 1080p, 8 at 3840 x 2160 -- where 16 would be 8.5 GB): per slot and pixel 16 B of z keys, 16 B of tie side words,
        // 32 B of triangle queue, with edge points 28 B of edge keys, their list and the vertex list, 3 B of filter flags
        ws_chunk = slots_afforded(c, nominal_slot_bytes(c->W, c->H, plan.edge_points, plan.remove_edges), ws_chunk);
    }
    // pure-shift mesh rows with edge removal: a launch is (frames x 135 bands) workgroups for 512 slots -- 8 frames
    // leave the chip 30 % idle in the last wave of workgroups (476 -> see DESIGN.md); the workspace is 11 B/px per frame
    // (points with edge removal likewise since r04: every launch set ends with k_edge_rows_exact, a handful of workgroups the
    //  stream waits for -- once per 32 frames instead of once per 8)
    if (!r.general) ws_chunk = 4 * kWorkspaceChunk;
    if (tuned_chunk) ws_chunk = tuned_chunk;
    if (r.general && ws_chunk > 32) ws_chunk = 32;        // one parity bit per z-key slot (uint32_t key_parity)
    return n < ws_chunk ? n : ws_chunk;
}

// The hole counts' per-row and per-wave counters of `frames` frames in flight, grown on demand.
static int ensure_count_buffers(mdvt_ctx* c, int frames, hipStream_t s)
{
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_ROW_COUNTS], (size_t)frames * 2 * c->H * sizeof(uint32_t), s));
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_WAVE_COUNTS], (size_t)frames * c->H * 16 * sizeof(uint32_t), s));
    return MDVT_OK;
}

// An earlier general-path submission stopped between splat and resolve: re-establish the EMPTY invariant the resolve pass normally maintains.
static int reset_dirty_keys(mdvt_ctx* c, const RenderWorkspaceLayout& L, hipStream_t s)
{
    for (int e = 0; e < 2; ++e) {
        if (c->keys[e]) MDVT_HIP(c, hipMemsetAsync(c->keys[e], 0xFF, L.plane_bytes(), s));
        if (c->ekeys[e]) MDVT_HIP(c, hipMemsetAsync(c->ekeys[e], 0xFF, L.plane_bytes(), s));
    }
    if (c->elist) MDVT_HIP(c, hipMemsetAsync(c->elist + L.elist_count_at(), 0, L.slots * L.H * sizeof(uint32_t), s));
    c->key_parity = 0;
    return MDVT_OK;
}

// Points RenderArgs at the workspace slots [slot0, ...) of a launch set: the whole workspace (slot0 = 0, bank 0) or a bank's half
// (slot0 = bank * bank_slots).  Allocates nothing: the second bank's separate huge list is made by submit_run.
static void bind_workspace(RenderArgs& a, const mdvt_ctx* c, const RenderWorkspaceLayout& L, int slot0, int bank, int bank_slots)
{
    const size_t s0 = (size_t)slot0;
    auto at = [](auto* p, size_t off) -> decltype(p) { return p ? p + off : nullptr; };
    for (int e = 0; e < 2; ++e) {
        a.keys[e] = at(c->keys[e], s0 * L.npx);
        a.ekeys[e] = at(c->ekeys[e], s0 * L.npx);
        a.cbuf[e] = at(c->cbuf[e], s0 * L.npx);
    }
    a.elist = at(c->elist, s0 * L.elist_stride());
    a.elist_count = at(c->elist, L.elist_count_at() + s0 * L.H);
    a.vlist = at(c->elist, L.vlist_at() + s0 * L.npx);
    a.vlist_count = at(c->elist, L.vlist_count_at() + s0);
    a.tri_invalid = at(c->tri_invalid, s0 * L.ntri);
    a.unused = at(c->unused, s0 * L.npx);
    if (!c->bigq) return;
    a.bigq = c->bigq + s0 * L.queue_stride(); a.bigq_cap = (uint32_t)L.bigq_cap();
    a.bigq_count = c->bigq + L.counters_at() + L.bank_counters_at(bank, bank_slots);      // (counters and prefix sums of a set; 16-byte aligned)
    // The second bank's own huge list: a separate allocation, made when banks are first used (r04: with both lists in the
    // queue's block a 100 x 31 frame's block passed 2 MB and left the runtime's fragment cache -- see the workspace pool above).
    a.hugeq = c->bigq + L.huge_at();      // (8-byte aligned: entries are uint2)
    if (bank) a.hugeq = L.huge_lists == 2 ? a.hugeq + L.huge_list_dwords() : c->hugeq2;
    a.tie_flag = c->bigq + L.tie_flag_at() + s0;
    a.tie_tiles = c->bigq + L.tie_tiles_at() + s0 * L.tie_tiles_stride();
    a.tie_words = (int32_t)L.tie_words; a.tie_tiles_x = (c->W + mdvt::kTieTile - 1) / mdvt::kTieTile;
}

// (every way out of the bank loop joins the side stream back into the caller's: an error return must not leave the side
//  stream working on its half of the workspace -- and on the caller's output buffers -- behind the caller's back; advisor, r04)
struct BankJoin {
    mdvt_ctx* c; hipStream_t s_call; bool armed;
    ~BankJoin() {
        if (!armed) return;
        if (hipEventRecord(c->ev_join, c->side) != hipSuccess || hipStreamWaitEvent(s_call, c->ev_join, 0) != hipSuccess) (void)hipStreamSynchronize(c->side);
    }
};

// One run's launch sets of up to `chunk` frames; `base`: everything of RenderArgs but the workspace.
static int submit_run(mdvt_ctx* c, RenderPlan plan, const Run& r, int chunk, const RenderArgs& base, const RenderWorkspaceLayout& L,
               const std::vector<FrameDev>& fd, const BatchFlags& bf, hipStream_t s_call)
{
    const int W = c->W, H = c->H;
    plan.general = r.general; plan.conv = r.conv; plan.conv_raster = r.craster;
    // Posed / converged mesh frames in more than one launch set: the sets take turns on two halves ("banks") of the workspace slots
    // and on two streams, a set starting when the vertex pass of the set before it is through -- the path's stages wait for
    // different things (the vertex pass for its stores, the rasteriser for its atomics), and the next set's vertex pass and edge
    // filter fill the rasteriser's waits: 32 frames of 1080p product default +3 %, mesh + convergence +4 %, mesh under a pose +7 %,
    // 8 frames of 4K pose + contention (C4) +10 %; a run that fits ONE launch set stays as it is (16 frames: two sets of 8 lose 1.5 %).
    // Points on the general path likewise (splat, then resolve: the next set's splat beside this set's resolve): C4 points +13 %.
    const bool bankable = r.general && !r.conv && !bf.want_bits && !base.hole_counts && tuning_env(TUNE_WS_CHUNK) == nullptr;
    bool banks = bankable && chunk >= 2 && r.f1 - r.f0 > chunk;
    int bank_slots = chunk / 2;
    // r05: a posed mesh run that FITS one launch set is split into two sets on the two banks all the same when each half is large
    // enough to fill the chip by itself (3 frames of 4K = 24.9 M pixels: 6 to 8 frames of C4's shape) -- since the vertex records went (64 B/px per slot, was 96) the
    // 8 frames of C4 are one set of 8 slots, and its cell walk (VALU) and resolve (HBM) ran one after the other again
    if (bankable && !banks && plan.mode == MDVT_MODE_MESH && r.f1 - r.f0 <= chunk && r.f1 - r.f0 >= 4 &&
        (size_t)((r.f1 - r.f0) / 2) * (size_t)W * (size_t)H >= (size_t)3 * 3840 * 2160) {
        banks = true;
        bank_slots = (r.f1 - r.f0) / 2;
    }
    BankJoin bank_join{c, s_call, false};
    if (banks) {
        chunk = bank_slots;
        if (!c->side) MDVT_HIP(c, bank_res_take(c));        // (process-wide: see bank_res_take)
        MDVT_HIP(c, hipEventRecord(c->ev_start, s_call));            // (the inputs, the parameter block, the runs before this one)
        MDVT_HIP(c, hipStreamWaitEvent(c->side, c->ev_start, 0));
        bank_join.armed = true;
    }
    int set = 0;
    for (int f0 = r.f0; f0 < r.f1; f0 += chunk, ++set) {
        plan.n = (r.f1 - f0 < chunk) ? r.f1 - f0 : chunk;
        const int bank = banks ? (set & 1) : 0, slot0 = bank * bank_slots;
        hipStream_t const s_set = bank ? c->side : s_call;
        if (bank && c->bigq && c->huge_lists != 2 && !c->hugeq2) MDVT_HIP(c, ws_malloc(c, (void**)&c->hugeq2, L.huge_list_dwords() * sizeof(uint32_t), s_set));
        RenderArgs a = base;
        bind_workspace(a, c, L, slot0, bank, bank_slots);
        if (banks) {
            if (set > 0) MDVT_HIP(c, hipStreamWaitEvent(s_set, c->ev_vert[bank ^ 1], 0));      // (the set before this one has projected its vertices / splatted its points)
            plan.after_vertices = c->ev_vert[bank];
        }
        a.frame0 = f0;
        if (plan.remove_edges) { if (int rc = filter_edges(c, a, plan.n, a.tri_invalid, a.unused, s_set)) return rc; }
        if (bf.no_byte_mask && !MDVT_GRID_CALL(c, points_fused_bits_applies, plan, a))
            return fail(c, MDVT_ERR_INVALID_ARG, "the byte masks may be NULL only where the mask compaction is fused into the render "
                        "(points mode, pure stereo shift, no edge removal, W %% 4 == 0, W <= 4096, dword-aligned image pointers, pitches and strides)");
        a.key_parity = c->key_parity >> slot0;
        plan.edge_rows_max = 0;
        if (!r.general && !r.conv && plan.edge_points)
            for (int k = f0; k < f0 + plan.n; ++k)
                if (fd[(size_t)k].erow_lo < fd[(size_t)k].erow_hi)
                    plan.edge_rows_max = std::max(plan.edge_rows_max, fd[(size_t)k].erow_hi - fd[(size_t)k].erow_lo + 1);
        hipError_t e = MDVT_GRID_CALL(c, launch_render, plan, a, s_set);
        plan.after_vertices = nullptr;
        if (r.general && e == hipSuccess) c->key_parity ^= (plan.n >= 32 ? 0xFFFFFFFFu : ((1u << plan.n) - 1u)) << slot0;   // these slots' next use has the other parity
        if (e == hipErrorNotSupported) return fail(c, MDVT_ERR_UNSUPPORTED, "render mode %d is not built yet", plan.mode);
        if (e != hipSuccess) return fail(c, MDVT_ERR_HIP, "render launch failed: %s", hipGetErrorString(e));
        if ((bf.want_bits || a.hole_counts) && !plan.fused_bits && plan.eyes != 1) MDVT_HIP(c, launch_pack_mask(a, plan.n, s_set));
        if (a.hole_counts && !plan.fused_bits && plan.eyes != 1) MDVT_HIP(c, launch_reduce_counts(a, plan.n, s_set));
    }
    if (banks) {
        MDVT_HIP(c, hipEventRecord(c->ev_join, c->side));
        MDVT_HIP(c, hipStreamWaitEvent(s_call, c->ev_join, 0));
        bank_join.armed = false;
    }
    return MDVT_OK;
}

static int render_frames(mdvt_ctx* c, int n_frames, std::vector<FrameDev>& fd, int any_general_frame, const mdvt_io* io, const BatchFlags& bf,
                         hipStream_t s, int eyes);

int mdvt_render_stereo_batch(mdvt_ctx* c, int n_frames, const mdvt_frame_params* params, const mdvt_io* io, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    BatchFlags bf{};
    int rc = validate_batch(c, n_frames, params, io, bf);
    if (rc != MDVT_OK) return rc;
    DeviceGuard g(c->device);
    hipStream_t const s = (hipStream_t)stream;
    std::vector<FrameDev> fd((size_t)n_frames);
    int any_general_frame = 0;
    for (int k = 0; k < n_frames; ++k) {
        if ((rc = fill_frame_dev(c, params[k], fd[(size_t)k])) != MDVT_OK) return rc;
        any_general_frame |= fd[(size_t)k].general;
        fd[(size_t)k].div_slot = -1;
    }
    if (c->cfg.samples == 4) return render_msaa(c, n_frames, fd, io, s);
    return render_frames(c, n_frames, fd, any_general_frame, io, bf, s, 2);
}

// The single-sample render of a validated batch.  eyes = 1: a view render (mdvt_render_view_batch) -- `io` carries eye 0's buffers in
// its left_* fields and NULL right_* ones, every frame is posed (general), io->hole_counts is one word per frame.
static int render_frames(mdvt_ctx* c, int n_frames, std::vector<FrameDev>& fd, int any_general_frame, const mdvt_io* io, const BatchFlags& bf,
                         hipStream_t s, int eyes)
{
    int rc;
    if (c->cfg.mode == MDVT_MODE_POINTS && (rc = assign_div_slots(c, fd, s)) != MDVT_OK) return rc;

    const FrameDev* dfp = nullptr;
    ParamSlot* slot = nullptr;
    if ((rc = stage_params(c, fd, s, &dfp, &slot)) != MDVT_OK) return rc;

    RenderPlan plan{};
    plan.mode = c->cfg.mode;
    plan.eyes = eyes;
    plan.remove_edges = c->cfg.remove_edges;
    plan.edge_points = c->cfg.remove_edges && c->cfg.edge_points;
    plan.general = any_general_frame;
    plan.allow_conv = c->opt_mesh_conv ? 1 : 0;
    if (tuning_build()) { const char* e = tuning_env(TUNE_MESH_CONV); plan.allow_conv = (e && e[0] == '1') ? 1 : 0; }   // (tests toggle it per call)
    plan.vec4 = (c->W % 4 == 0) && aligned(io->depth_rgb, 4) && aligned(io->color_rgb, 4) && aligned(io->left_rgb, 4) &&
                aligned(io->right_rgb, 4) && aligned(io->left_mask, 4) && aligned(io->right_mask, 4) &&
                io->depth_pitch % 4 == 0 && io->color_pitch % 4 == 0 && io->rgb_pitch % 4 == 0 && io->mask_pitch % 4 == 0 &&
                io->depth_stride % 4 == 0 && io->color_stride % 4 == 0 && io->rgb_stride % 4 == 0 && io->mask_stride % 4 == 0 &&
                (!io->left_seed || (aligned(io->left_seed, 4) && aligned(io->right_seed, 4) && io->seed_pitch % 4 == 0 && io->seed_stride % 4 == 0)) &&
                (!bf.zout || ((!io->left_depth || aligned(io->left_depth, 16)) && (!io->right_depth || aligned(io->right_depth, 16)) &&
                              io->zout_pitch % 16 == 0 && io->zout_stride % 16 == 0));

    std::vector<Run> runs;
    build_runs(c, plan, fd, runs);
    bool any_global = false, uses_global_ws = false;          // some run takes the global-key kernels / uses the global workspace
    for (const Run& r : runs) { any_global |= r.general != 0; uses_global_ws |= r.general || r.conv; }
    int tuned_chunk = 0;
    if (const char* e = tuning_env(TUNE_WS_CHUNK)) { const int v = atoi(e); if (v > 0) tuned_chunk = v; }   // tuning hook
    int ws_frames = 0, count_frames = 0;
    for (const Run& r : runs) {
        const int ch = chunk_of(c, plan, r, tuned_chunk);
        if ((r.general || r.conv || plan.remove_edges) && ch > ws_frames) ws_frames = ch;
        if (ch > count_frames) count_frames = ch;
    }
    if (ws_frames && (rc = ensure_workspace(c, ws_frames, any_global, uses_global_ws && plan.edge_points, plan.remove_edges,
                                            any_global && plan.mode == MDVT_MODE_MESH, s, eyes)) != MDVT_OK) return rc;
    RenderArgs base{};
    bind_io(base, c, io, dfp);
    base.zout[0] = io->left_depth; base.zout[1] = io->right_depth; base.zout_pitch = io->zout_pitch; base.zout_stride = io->zout_stride;
    base.maskbits[0] = io->left_maskbits; base.maskbits[1] = io->right_maskbits;
    base.maskbits_pitch = io->maskbits_pitch; base.maskbits_stride = io->maskbits_stride;
    base.seed[0] = io->left_seed; base.seed[1] = io->right_seed; base.seed_pitch = io->seed_pitch; base.seed_stride = io->seed_stride;
    if (io->hole_counts && eyes == 1) MDVT_HIP(c, hipMemsetAsync(io->hole_counts, 0, (size_t)n_frames * sizeof(uint32_t), s));      // (the view resolve adds to them)
    if (io->hole_counts && eyes == 2) {
        if ((rc = ensure_count_buffers(c, count_frames, s)) != MDVT_OK) return rc;
        base.row_counts = c->scratch[SCR_ROW_COUNTS].as<uint32_t>(); base.wave_counts = c->scratch[SCR_WAVE_COUNTS].as<uint32_t>();
    }
    base.divcheck = c->divcheck; base.edge_paint = c->cfg.edge_points != 2; base.cull = c->cfg.cull;
    if (c->cfg.mode == MDVT_MODE_MESH) { if ((rc = ensure_rowcell(c, s)) != MDVT_OK) return rc; base.rowcell = c->rowcell; }
    const RenderWorkspaceLayout L = layout_of(c);
    // (the z keys' parity is kept per slot for both eyes: after view renders eye 1's planes lag behind, and a stereo render starts from
    //  planes reset to parity 0, as after an interrupted submission)
    if (uses_global_ws && (c->keys_dirty || (eyes == 2 && c->eye1_stale)) && (rc = reset_dirty_keys(c, L, s)) != MDVT_OK) return rc;
    if (uses_global_ws) { c->keys_dirty = true; c->eye1_stale = eyes == 1 && c->keys[1] != nullptr; }
    for (const Run& r : runs)
        if ((rc = submit_run(c, plan, r, chunk_of(c, plan, r, tuned_chunk), base, L, fd, bf, s)) != MDVT_OK) return rc;
    if (uses_global_ws) c->keys_dirty = false;
    if (bf.near_clip && (rc = render_near_clip_gate(c, n_frames, dfp, io, s)) != MDVT_OK) return rc;
    MDVT_HIP(c, hipEventRecord(slot->done, s));
    return MDVT_OK;
}

int mdvt_render_stereo(mdvt_ctx* c, const mdvt_frame_params* params, const mdvt_io* io, void* stream)
{
    return mdvt_render_stereo_batch(c, 1, params, io, stream);
}

int mdvt_debug_read(mdvt_ctx* c, int what, void* h_dst, uint64_t capacity, uint64_t info[8])
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!tuning_build()) return fail(c, MDVT_ERR_UNSUPPORTED, "mdvt_debug_read: tuning build only");
    if (what < 0 || what > 2 || !info) return fail(c, MDVT_ERR_INVALID_ARG, "mdvt_debug_read: what must be 0, 1 or 2, info not NULL");
    if (what == 2) {
        // the two process-wide pools as this context's GPU sees them (its pool tag: the device, or MDVT_POOL_TAG): idle parameter
        // blocks that carry device memory of this / of another GPU, idle workspace blocks of this / of another GPU
        for (int k = 0; k < 8; ++k) info[k] = 0;
        pool_idle_blocks(c->pool_tag, info);
        info[4] = (uint64_t)c->pool_tag;
        return MDVT_OK;
    }
    DeviceGuard g(c->device);
    MDVT_HIP(c, hipDeviceSynchronize());
    if (what == 1) {
        // the coherence test of mdvt_selftest.hip on the queue block itself (it OVERWRITES the block: the next render rewrites what it
        // reads): h_dst receives 80 dwords; info[0] = the tag used
        if (!c->bigq || !h_dst || capacity < 80 * sizeof(uint32_t)) return fail(c, MDVT_ERR_INVALID_ARG, "mdvt_debug_read: no queue block / 320 bytes needed");
        static uint32_t tag = 0x1234567u;
        tag = tag * 1664525u + 1013904223u;
        uint32_t *d_xcc = nullptr, *d_out = nullptr;
        MDVT_HIP(c, hipMalloc((void**)&d_xcc, (c->bigq_bytes / 256 + 1) * sizeof(uint32_t)));
        MDVT_HIP(c, hipMalloc((void**)&d_out, 80 * sizeof(uint32_t)));
        hipError_t e = launch_coherence_test(c->bigq, c->bigq_bytes / 4, tag, d_xcc, d_out, nullptr);
        if (e == hipSuccess) e = hipMemcpy(h_dst, d_out, 80 * sizeof(uint32_t), hipMemcpyDeviceToHost);
        (void)hipFree(d_xcc); (void)hipFree(d_out);
        if (e != hipSuccess) return fail(c, MDVT_ERR_HIP, "mdvt_debug_read: %s", hipGetErrorString(e));
        info[0] = tag;
        return MDVT_OK;
    }
    const RenderWorkspaceLayout L = layout_of(c);
    info[0] = c->bigq ? c->bigq_bytes : 0;                                   // bytes of the queue block
    info[1] = c->bigq_counters_at;                                           // dword offset of the segment counters (as the block was made)
    info[2] = L.slots * L.H;                                                 // segments the block has room for
    info[3] = info[1] + L.counter_words();                                   // dword offset of the (first) huge list
    info[4] = info[3] + L.huge_lists * L.huge_list_dwords();                 // dword offset of the tie flags
    info[5] = (uint64_t)c->W; info[6] = (uint64_t)c->H; info[7] = (uint64_t)c->ws_frames;
    if (h_dst && c->bigq) {
        if (capacity < c->bigq_bytes) return fail(c, MDVT_ERR_INVALID_ARG, "mdvt_debug_read: %zu bytes needed", c->bigq_bytes);
        MDVT_HIP(c, hipMemcpy(h_dst, c->bigq, c->bigq_bytes, hipMemcpyDeviceToHost));
    }
    return MDVT_OK;
}

int mdvt_edge_point_pixels(mdvt_ctx* c, const mdvt_frame_params* params, const uint8_t* d_depth_rgb, size_t depth_pitch,
                           int how, int32_t* d_px, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!c->cfg_set) return fail(c, MDVT_ERR_INVALID_ARG, "mdvt_set_config has not been called");
    if (!params || !d_depth_rgb || !d_px) return fail(c, MDVT_ERR_INVALID_ARG, "NULL argument");
    if (depth_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (how != 0 && how != 1) return fail(c, MDVT_ERR_INVALID_ARG, "how must be 0 (the chain) or 1 (as the row kernels take it)");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    std::vector<FrameDev> fd(1);
    // (the row range is only worked out for configurations that splat edge points; this entry point always wants it)
    mdvt_config saved = c->cfg;
    c->cfg.remove_edges = 1; c->cfg.edge_points = 1;
    const int rc0 = fill_frame_dev(c, *params, fd[0]);
    c->cfg = saved;
    if (rc0 != MDVT_OK) return rc0;
    if (how == 1 && (fd[0].general || fd[0].erow_wild))
        return fail(c, MDVT_ERR_INVALID_ARG, "how = 1 needs a pure-shift frame whose rows the row kernels take");
    const FrameDev* dfp = nullptr;
    ParamSlot* slot = nullptr;
    const int rc = stage_params(c, fd, s, &dfp, &slot);
    if (rc != MDVT_OK) return rc;
    MDVT_HIP(c, launch_edge_point_pixels(d_depth_rgb, depth_pitch, dfp, c->W, c->H, c->cfg.mode == MDVT_MODE_MESH ? 1 : 0, how, d_px, s));
    MDVT_HIP(c, hipEventRecord(slot->done, s));
    return MDVT_OK;
}

int mdvt_edge_filter(mdvt_ctx* c, const uint8_t* d_depth_rgb, size_t depth_pitch, const double K[9], double depth_scale,
                     int of_by_one, uint8_t* d_tri_invalid, uint8_t* d_unused, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_depth_rgb || !K) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (depth_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (c->W < 2 || c->H < 2) return fail(c, MDVT_ERR_INVALID_ARG, "the edge filter needs at least a 2x2 frame");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    std::vector<FrameDev> fd(1);
    FrameDev& f = fd[0];
    memset(&f, 0, sizeof f);
    f.mult = (float)(c->cfg.max_depth / 4228250625.0);
    f.scale = (float)depth_scale;
    f.Kd[0] = K[0]; f.Kd[1] = K[4]; f.Kd[2] = K[2]; f.Kd[3] = K[5];
    f.rKd[0] = 1.0 / K[0]; f.rKd[1] = 1.0 / K[4];
    const FrameDev* dfp = nullptr;
    ParamSlot* slot = nullptr;
    int rc = stage_params(c, fd, s, &dfp, &slot);
    if (rc != MDVT_OK) return rc;
    if (d_unused) MDVT_HIP(c, hipMemsetAsync(d_unused, 0, (size_t)c->W * c->H, s));
    MDVT_HIP(c, launch_edge_filter(d_depth_rgb, depth_pitch, 0, dfp, 0, 1, c->W, c->H, of_by_one ? 1 : 0,
                                   d_tri_invalid, 0, d_unused, 0, s));
    MDVT_HIP(c, hipEventRecord(slot->done, s));
    return MDVT_OK;
}

// The per-frame centre of the vertices (mdvt_view.hip).  Launch sets: as many frames as the ctx's workspace budget affords.
int mdvt_view_centers(mdvt_ctx* c, int n_frames, const mdvt_frame_params* params, const uint8_t* d_depth_rgb, size_t depth_pitch,
                      size_t depth_stride, double* d_centers, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!c->cfg_set) return fail(c, MDVT_ERR_INVALID_ARG, "mdvt_set_config has not been called");
    if (n_frames < 1 || !params) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames/params invalid");
    if (!d_depth_rgb || !d_centers) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (!aligned(d_centers, 8)) return fail(c, MDVT_ERR_INVALID_ARG, "d_centers must be 8-byte aligned");
    const int W = c->W, H = c->H;
    if (depth_pitch < (size_t)3 * W) return fail(c, MDVT_ERR_INVALID_ARG, "depth_pitch smaller than one row");
    if (n_frames > 1 && depth_stride < depth_pitch * (size_t)H) return fail(c, MDVT_ERR_INVALID_ARG, "depth_stride smaller than one frame");
    const bool park = c->cfg.mode == MDVT_MODE_POINTS && c->cfg.remove_edges;
    if (park && (W < 2 || H < 2)) return fail(c, MDVT_ERR_INVALID_ARG, "the edge filter needs at least a 2x2 frame");
    if ((uint64_t)W * (uint64_t)H > ((uint64_t)1 << 28)) return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large for the centres (%d x %d)", W, H);
    std::vector<FrameDev> fd((size_t)n_frames);
    for (int k = 0; k < n_frames; ++k) {
        if (int rc = fill_frame_dev(c, params[k], fd[(size_t)k])) return rc;
        fd[(size_t)k].div_slot = -1;
    }
    DeviceGuard g(c->device);
    hipStream_t const s = (hipStream_t)stream;
    const uint32_t npx = (uint32_t)W * (uint32_t)H, nchunks = (npx + 8191u) / 8192u;
    const size_t sums_bytes = up16((size_t)nchunks * mdvt::kViewSumBytes), flag_bytes = park ? up16((size_t)npx) : 0;
    const int fchunk = slots_afforded(c, sums_bytes + flag_bytes, n_frames < 4096 ? n_frames : 4096);
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_VIEW], (size_t)fchunk * (sums_bytes + flag_bytes), s));
    const FrameDev* dfp = nullptr;
    ParamSlot* slot = nullptr;
    if (int rc = stage_params(c, fd, s, &dfp, &slot)) return rc;
    mdvt::ViewCentersArgs a{};
    a.depth = d_depth_rgb; a.depth_pitch = depth_pitch; a.depth_stride = depth_stride;
    a.fp = dfp; a.W = W; a.H = H; a.of_by_one = c->cfg.mode == MDVT_MODE_MESH ? 1 : 0;
    a.npx = npx; a.nchunks = nchunks;
    a.sums = c->scratch[SCR_VIEW].as<double>();
    uint8_t* const flags = park ? c->scratch[SCR_VIEW].p + (size_t)fchunk * sums_bytes : nullptr;
    a.unused = flags; a.unused_stride = flag_bytes;
    a.centers = d_centers;
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        a.frame0 = f0;
        a.n_frames = set_len(n_frames, f0, fchunk);
        if (park) {
            MDVT_HIP(c, launch_zero_bytes(flags, (size_t)a.n_frames * flag_bytes, s));
            MDVT_HIP(c, launch_edge_filter(d_depth_rgb, depth_pitch, depth_stride, dfp, f0, a.n_frames, W, H, 0, nullptr, 0, flags, flag_bytes, s));
        }
        MDVT_HIP(c, mdvt::launch_view_centers(a, s));
    }
    MDVT_HIP(c, hipEventRecord(slot->done, s));
    return MDVT_OK;
}

// The geometry export (include/mdvt_geometry.h; mdvt_geometry.hip).  Launch sets: as many frames as the ctx's workspace budget affords.
int mdvt_export_geometry_batch(mdvt_ctx* c, int n_frames, const mdvt_frame_params* params, const mdvt_geometry_opts* opts,
                               const mdvt_geometry_io* io, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (n_frames < 1 || !params || !opts || !io) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames/params/opts/io invalid");
    if (!io->depth_rgb || !io->counts) return fail(c, MDVT_ERR_INVALID_ARG, "depth_rgb and counts are required");
    if (io->point_rgb && !io->color_rgb) return fail(c, MDVT_ERR_INVALID_ARG, "point_rgb needs color_rgb");
    const int W = c->W, H = c->H;
    if (W < 2 || H < 2) return fail(c, MDVT_ERR_INVALID_ARG, "the geometry export needs at least a 2x2 frame");
    if ((uint64_t)W * (uint64_t)H > ((uint64_t)1 << 28)) return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large for the geometry export (%d x %d)", W, H);
    if (opts->decode != 0 && opts->decode != 1) return fail(c, MDVT_ERR_UNSUPPORTED, "decode must be 0 (the exporter's) or 1 (the render's)");
    if (opts->reserved[0] || opts->reserved[1]) return fail(c, MDVT_ERR_UNSUPPORTED, "mdvt_geometry_opts.reserved must be 0");
    if (!(opts->max_depth > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "max_depth must be > 0");
    const size_t N = (size_t)W * (size_t)H, ncell = (size_t)(W - 1) * (size_t)(H - 1);
    if (io->depth_pitch < (size_t)3 * W || (io->color_rgb && io->color_pitch < (size_t)3 * W)) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    const bool many = n_frames > 1;
    if (many && (io->depth_stride < io->depth_pitch * (size_t)H || (io->color_rgb && io->color_stride < io->color_pitch * (size_t)H)))
        return fail(c, MDVT_ERR_INVALID_ARG, "input stride smaller than one frame");
    if (many && ((io->vertices && io->vertices_stride < 24 * N) || (io->triangles && io->triangles_stride < 24 * ncell) ||
                 (io->used_index && io->used_stride < 4 * N) || (io->points && io->points_stride < 24 * N) ||
                 (io->point_rgb && io->point_rgb_stride < 3 * N)))
        return fail(c, MDVT_ERR_INVALID_ARG, "output stride smaller than a full frame's list");
    if (!aligned(io->vertices, 8) || !aligned(io->points, 8) || (many && ((io->vertices && io->vertices_stride % 8) || (io->points && io->points_stride % 8))))
        return fail(c, MDVT_ERR_INVALID_ARG, "vertices and points (and their strides) must be 8-byte aligned");
    if (!aligned(io->triangles, 4) || !aligned(io->used_index, 4) || !aligned(io->counts, 4) ||
        (many && ((io->triangles && io->triangles_stride % 4) || (io->used_index && io->used_stride % 4))))
        return fail(c, MDVT_ERR_INVALID_ARG, "triangles, used_index and counts (and their strides) must be 4-byte aligned");
    std::vector<FrameDev> fd((size_t)n_frames);
    for (int k = 0; k < n_frames; ++k) {
        const mdvt_frame_params& p = params[k];
        FrameDev& f = fd[(size_t)k];
        if (!(p.K[0] > 0.0) || !(p.K[4] > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "camera matrix needs positive focal lengths");
        if (!(p.depth_scale > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "depth_scale must be > 0");
        if (p.has_T && (fabs(p.T[12]) > 1e-12 || fabs(p.T[13]) > 1e-12 || fabs(p.T[14]) > 1e-12 || fabs(p.T[15] - 1.0) > 1e-12))
            return fail(c, MDVT_ERR_UNSUPPORTED, "pose matrix must be affine (last row 0 0 0 1)");
        memset(&f, 0, sizeof f);
        f.mult = opts->decode ? (float)(opts->max_depth / 4228250625.0) : (float)(4228250625.0 / opts->max_depth);       // dfh:22; cmf:652 (the divisor)
        f.scale = (float)p.depth_scale;
        f.sx = (float)(((double)W + 1.0) / (double)W);
        f.sy = (float)(((double)H + 1.0) / (double)H);
        f.Kd[0] = p.K[0]; f.Kd[1] = p.K[4]; f.Kd[2] = p.K[2]; f.Kd[3] = p.K[5];
        f.rKd[0] = 1.0 / p.K[0]; f.rKd[1] = 1.0 / p.K[4];
        f.has_T = p.has_T ? 1 : 0;
        if (p.has_T) memcpy(f.Td, p.T, sizeof f.Td);
        f.div_slot = -1;
    }
    DeviceGuard g(c->device);
    hipStream_t const s = (hipStream_t)stream;
    mdvt::GeometryArgs a{};
    a.npx = (uint32_t)N; a.ncell = (uint32_t)ncell;
    a.nbt = (uint32_t)((2 * ncell + mdvt::kGeomBlock - 1) / mdvt::kGeomBlock);
    a.nbv = (uint32_t)((N + mdvt::kGeomBlock - 1) / mdvt::kGeomBlock);
    const size_t flag_bytes = opts->remove_edges ? up16(2 * ncell) : 0, total_bytes = up16(((size_t)a.nbt + a.nbv) * sizeof(uint32_t));
    const int fchunk = slots_afforded(c, flag_bytes + total_bytes, n_frames < 4096 ? n_frames : 4096);
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_GEOMETRY], (size_t)fchunk * (flag_bytes + total_bytes), s));
    const FrameDev* dfp = nullptr;
    ParamSlot* slot = nullptr;
    if (int rc = stage_params(c, fd, s, &dfp, &slot)) return rc;
    a.depth = io->depth_rgb; a.depth_pitch = io->depth_pitch; a.depth_stride = io->depth_stride;
    a.color = io->color_rgb; a.color_pitch = io->color_pitch; a.color_stride = io->color_stride;
    a.vertices = io->vertices; a.vertices_stride = io->vertices_stride;
    a.triangles = io->triangles; a.triangles_stride = io->triangles_stride;
    a.used_index = io->used_index; a.used_stride = io->used_stride;
    a.points = io->points; a.points_stride = io->points_stride;
    a.point_rgb = io->point_rgb; a.point_rgb_stride = io->point_rgb_stride;
    a.counts = io->counts;
    a.fp = dfp; a.W = W; a.H = H; a.decode = opts->decode;
    a.totals = c->scratch[SCR_GEOMETRY].as<uint32_t>();
    a.flags = opts->remove_edges ? c->scratch[SCR_GEOMETRY].p + (size_t)fchunk * total_bytes : nullptr;
    a.flags_stride = flag_bytes;
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        a.frame0 = f0;
        a.n_frames = set_len(n_frames, f0, fchunk);
        MDVT_HIP(c, mdvt::launch_export_geometry(a, s));
    }
    MDVT_HIP(c, hipEventRecord(slot->done, s));
    return MDVT_OK;
}

// The grey depth of cmf:752-760 (include/mdvt_geometry.h): no workspace, no frame parameters.
int mdvt_depth_grey_batch(mdvt_ctx* c, int n_frames, const uint8_t* d_depth_rgb, size_t pitch, size_t stride, double max_depth, int bits,
                          void* d_out, size_t out_pitch, size_t out_stride, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (n_frames < 1 || !d_depth_rgb || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames/buffers invalid");
    if (bits != 8 && bits != 16) return fail(c, MDVT_ERR_INVALID_ARG, "bits must be 8 or 16");
    if (!(max_depth > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "max_depth must be > 0");
    const int W = c->W, H = c->H;
    const size_t out_row = bits == 16 ? (size_t)2 * W : (size_t)3 * W;
    if (pitch < (size_t)3 * W || out_pitch < out_row) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (n_frames > 1 && (stride < pitch * (size_t)H || out_stride < out_pitch * (size_t)H)) return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if (bits == 16 && (!aligned(d_out, 2) || (H > 1 && out_pitch % 2) || (n_frames > 1 && out_stride % 2)))
        return fail(c, MDVT_ERR_INVALID_ARG, "a 16-bit output (its pitch and stride) must be 2-byte aligned");
    if ((uint64_t)W * (uint64_t)H > ((uint64_t)1 << 28)) return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large for the grey depth (%d x %d)", W, H);
    DeviceGuard g(c->device);
    const float divisor = (float)(4228250625.0 / max_depth);                                              // cmf:652
    const float mult = bits == 16 ? (float)(65025.0 / max_depth) : (float)(255.0 / max_depth);            // cmf:753, 757
    MDVT_HIP(c, mdvt::launch_depth_grey(d_depth_rgb, pitch, stride, divisor, mult, bits, d_out, out_pitch, out_stride, W, H, n_frames, (hipStream_t)stream));
    return MDVT_OK;
}

// One image per frame from the composed matrix in params[k].T (include/mdvt_view.h): the left eye of the stereo render with ipd_m = 0
// and no convergence, by the one-eye instantiations of the general kernels.
int mdvt_render_view_batch(mdvt_ctx* c, int n_frames, const mdvt_frame_params* params, const mdvt_view_io* vio, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!c->cfg_set) return fail(c, MDVT_ERR_INVALID_ARG, "mdvt_set_config has not been called");
    if (n_frames <= 0 || !params || !vio) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames/params/io invalid");
    if (!vio->depth_rgb || !vio->color_rgb || !vio->rgb) return fail(c, MDVT_ERR_INVALID_ARG, "depth_rgb, color_rgb and rgb are required");
    const char* what = nullptr;
    if (c->cfg.edge_points) what = "edge points (mdvt_config.edge_points != 0)";
    else if (c->cfg.samples == 4) what = "multisampling (samples = 4)";
    else if (c->near_clip) what = "near-plane clipping (mdvt_set_near_clip)";
    if (what) return fail(c, MDVT_ERR_UNSUPPORTED, "the view render does not cover %s", what);
    const int W = c->W, H = c->H;
    if (W < 2 || H < 2) return fail(c, MDVT_ERR_INVALID_ARG, "rendering needs at least a 2x2 frame");
    if (vio->depth_pitch < (size_t)3 * W || vio->color_pitch < (size_t)3 * W || vio->rgb_pitch < (size_t)3 * W ||
        (vio->mask && vio->mask_pitch < (size_t)W) || (vio->depth && vio->zout_pitch < (size_t)4 * W))
        return fail(c, MDVT_ERR_INVALID_ARG, "a pitch is smaller than one row");
    if (n_frames > 1 && (vio->depth_stride < vio->depth_pitch * (size_t)H || vio->color_stride < vio->color_pitch * (size_t)H ||
                         vio->rgb_stride < vio->rgb_pitch * (size_t)H || (vio->mask && vio->mask_stride < vio->mask_pitch * (size_t)H) ||
                         (vio->depth && vio->zout_stride < vio->zout_pitch * (size_t)H)))
        return fail(c, MDVT_ERR_INVALID_ARG, "a stride is smaller than one frame");
    if ((vio->depth && !aligned(vio->depth, 4)) || (vio->depth && (vio->zout_pitch % 4 || vio->zout_stride % 4)) || (vio->hole_counts && !aligned(vio->hole_counts, 4)))
        return fail(c, MDVT_ERR_INVALID_ARG, "the depth plane and the hole counts must be dword aligned");
    for (int k = 0; k < n_frames; ++k)
        if (!params[k].has_T) return fail(c, MDVT_ERR_INVALID_ARG, "frame %d: a view render takes the composed matrix V * T in T (has_T = 1)", k);
    std::vector<FrameDev> fd((size_t)n_frames);
    const double ipd = c->cfg.ipd_m;
    c->cfg.ipd_m = 0.0;                       // (ignored here, as convergence_angle is: both eye matrices are T)
    int rc = MDVT_OK;
    for (int k = 0; k < n_frames && rc == MDVT_OK; ++k) {
        mdvt_frame_params p = params[k];
        p.convergence_angle = 0.0;
        rc = fill_frame_dev(c, p, fd[(size_t)k]);
        fd[(size_t)k].div_slot = -1;
    }
    c->cfg.ipd_m = ipd;
    if (rc != MDVT_OK) return rc;
    mdvt_io io{};
    io.depth_rgb = vio->depth_rgb; io.depth_pitch = vio->depth_pitch; io.depth_stride = vio->depth_stride;
    io.color_rgb = vio->color_rgb; io.color_pitch = vio->color_pitch; io.color_stride = vio->color_stride;
    io.left_rgb = vio->rgb; io.rgb_pitch = vio->rgb_pitch; io.rgb_stride = vio->rgb_stride;
    io.left_mask = vio->mask; io.mask_pitch = vio->mask ? vio->mask_pitch : 0; io.mask_stride = vio->mask ? vio->mask_stride : 0;
    io.left_depth = vio->depth; io.zout_pitch = vio->zout_pitch; io.zout_stride = vio->zout_stride;
    io.hole_counts = vio->hole_counts;
    BatchFlags bf{};
    bf.zout = vio->depth != nullptr;
    DeviceGuard g(c->device);
    return render_frames(c, n_frames, fd, 1, &io, bf, (hipStream_t)stream, 1);
}

}  // extern "C"
