// mdvt_api_inspatio.hip -- the entry points of include/mdvt_inspatio.h: the 4 x 4 grid of masked cross-correlation shifts and the flow warp (kernels:
// mdvt_inspatio.hip).  The refusals stand in the order the caller meets their texts, each fail(...) text at its check; the layout
// tests, set loops and the scratch carver are mdvt_context.h's.  Host code only.
#include "mdvt_context.h"
#include "mdvt_inspatio.h"

using namespace mdvt;
using namespace mdvt::host;

namespace {

inline int quarter_up(int n) { return (n + 3) / 4; }               // the largest of the four cells of an axis: n - 3 * n / 4
inline bool size_refused(int width, int height) { return width < 8 || height < 8 || quarter_up(width) > kShiftMaxCell || quarter_up(height) > kShiftMaxCell; }
inline int log2_at_least(int n)
{
    int l = 2;                                                      // (a line of the transform has at least four values)
    while ((1 << l) < n) ++l;
    return l;
}

}  // namespace

extern "C" {

int mdvt_masked_shift_path(int width, int height)
{
    if (size_refused(width, height)) return 0;
    return quarter_up(width) * quarter_up(height) <= kShiftAutoDirectPixels ? MDVT_SHIFT_PATH_DIRECT : MDVT_SHIFT_PATH_TRANSFORM;
}

// One scratch block: the cells' state, the largest rounding distance, the planes of a launch set's interior cells.
int mdvt_masked_shift_grid(mdvt_ctx* c, int width, int height, int n_frames, const uint8_t* d_render, size_t render_pitch, size_t render_stride,
                           const uint8_t* d_infilled, size_t infilled_pitch, size_t infilled_stride,
                           const uint8_t* d_valid, size_t valid_pitch, size_t valid_stride,
                           int path, double* d_shift, uint8_t* d_status, uint64_t* d_round_error, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_render || !d_infilled || !d_valid || !d_shift || !d_status) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (!multiples_of(8, d_shift, d_round_error)) return fail(c, MDVT_ERR_INVALID_ARG, "d_shift and d_round_error must be 8-byte aligned");
    if (width < 1 || height < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d", width, height);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (render_pitch < (size_t)width * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "render_pitch smaller than one row");
    if (infilled_pitch < (size_t)width * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "infilled_pitch smaller than one row");
    if (valid_pitch < (size_t)width) return fail(c, MDVT_ERR_INVALID_ARG, "valid_pitch smaller than one row");
    if (n_frames > 1 && (render_stride < render_pitch * (size_t)height || infilled_stride < infilled_pitch * (size_t)height ||
                         valid_stride < valid_pitch * (size_t)height))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if (path != MDVT_SHIFT_PATH_AUTO && path != MDVT_SHIFT_PATH_DIRECT && path != MDVT_SHIFT_PATH_TRANSFORM)
        return fail(c, MDVT_ERR_INVALID_ARG, "path must be 0 (auto), 1 (direct) or 2 (transform), got %d", path);
    if (width < 8 || height < 8) return fail(c, MDVT_ERR_UNSUPPORTED, "an eye below 8 x 8 (%d x %d)", width, height);
    if (size_refused(width, height)) return fail(c, MDVT_ERR_UNSUPPORTED, "a cell side above %d (%d x %d)", kShiftMaxCell, width, height);
    if (n_frames > (1 << 24)) return fail(c, MDVT_ERR_UNSUPPORTED, "more than %d frames in one call", 1 << 24);
    const int hmax = quarter_up(height), wmax = quarter_up(width);
    if (path == MDVT_SHIFT_PATH_AUTO) path = mdvt_masked_shift_path(width, height);
    if (path == MDVT_SHIFT_PATH_DIRECT && hmax * wmax > kShiftDirectPixels)
        return fail(c, MDVT_ERR_UNSUPPORTED, "the direct path holds a cell of at most %d pixels in LDS (%d x %d)", kShiftDirectPixels, wmax, hmax);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) render_stride = infilled_stride = valid_stride = 0;
    mdvt::ShiftGridArgs a{};
    a.render = d_render; a.render_pitch = render_pitch; a.render_stride = render_stride;
    a.infilled = d_infilled; a.infilled_pitch = infilled_pitch; a.infilled_stride = infilled_stride;
    a.valid = d_valid; a.valid_pitch = valid_pitch; a.valid_stride = valid_stride;
    a.W = width; a.H = height; a.n_frames = n_frames; a.hmax = hmax; a.wmax = wmax;
    a.transform = path == MDVT_SHIFT_PATH_TRANSFORM;
    if (a.transform) {
        a.log_ly = log2_at_least(2 * hmax - 1); a.log_lx = log2_at_least(2 * wmax - 1);
        a.Ly = 1 << a.log_ly; a.Lx = 1 << a.log_lx;
    } else {
        a.Ly = 2 * hmax - 1; a.Lx = 2 * wmax - 1;
    }
    a.plane = (size_t)a.Ly * (size_t)a.Lx;
    const size_t state_bytes = up16((size_t)n_frames * 16u * sizeof(mdvt::ShiftCellState)) + 16u;
    const size_t unit_bytes = 3u * a.plane * sizeof(double2);
    const int units = 8 * n_frames;
    const int per_set = slots_afforded(c, unit_bytes, units < kGridFrames ? units : kGridFrames);
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_INSPATIO], state_bytes + (size_t)per_set * unit_bytes, s));
    uint8_t* w = c->scratch[SCR_INSPATIO].p;
    a.state = take<mdvt::ShiftCellState>(w, state_bytes - 16u);
    a.round_err = take<unsigned long long>(w, 16u);
    a.planes = take<double2>(w, (size_t)per_set * unit_bytes);
    a.round_err_out = reinterpret_cast<unsigned long long*>(d_round_error);
    a.shift = d_shift; a.status = d_status;
    MDVT_HIP(c, hipMemsetAsync(a.state, 0, state_bytes, s));
    MDVT_HIP(c, mdvt::launch_shift_gate(a, s));
    for (int u0 = 0; u0 < units; u0 += per_set) {
        a.unit0 = u0; a.n_units = set_len(units, u0, per_set);
        MDVT_HIP(c, mdvt::launch_shift_units(a, s));
    }
    MDVT_HIP(c, mdvt::launch_shift_finish(a, s));
    return MDVT_OK;
}

// No scratch block: launches only.
int mdvt_flow_warp(mdvt_ctx* c, int width, int height, int n_frames, const float* d_grids, const uint8_t* d_has_grid,
                   const uint8_t* d_infilled, size_t infilled_pitch, size_t infilled_stride, uint8_t* d_out, size_t out_pitch, size_t out_stride,
                   void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_grids || !d_has_grid || !d_infilled || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (!multiples_of(4, d_grids)) return fail(c, MDVT_ERR_INVALID_ARG, "d_grids must be 4-byte aligned");
    if (width < 1 || height < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d", width, height);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (infilled_pitch < (size_t)width * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "infilled_pitch smaller than one row");
    if (out_pitch < (size_t)width * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "out_pitch smaller than one row");
    if (n_frames > 1 && (infilled_stride < infilled_pitch * (size_t)height || out_stride < out_pitch * (size_t)height))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if ((uint64_t)width * (uint64_t)height >= ((uint64_t)1 << 31)) return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large (%d x %d)", width, height);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) infilled_stride = out_stride = 0;
    mdvt::FlowWarpArgs a{};
    a.grids = d_grids; a.has_grid = d_has_grid; a.src = d_infilled; a.src_pitch = infilled_pitch; a.src_stride = infilled_stride;
    a.dst = d_out; a.dst_pitch = out_pitch; a.dst_stride = out_stride; a.W = width; a.H = height;
    for (int f0 = 0; f0 < n_frames; f0 += kGridFrames) {
        a.frame0 = f0;
        MDVT_HIP(c, mdvt::launch_flow_warp(a, set_len(n_frames, f0, kGridFrames), s));
    }
    return MDVT_OK;
}

// No scratch block: one memset and two launches per set.
int mdvt_inspatio_prepare_eye(mdvt_ctx* c, int eye_w, int eye_h, int n_frames, int eye, const uint8_t* d_color, size_t color_pitch, size_t color_stride,
                              const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride, int model_w, int model_h,
                              uint8_t* d_valid, size_t valid_pitch, size_t valid_stride, uint8_t* d_render, size_t render_pitch, size_t render_stride,
                              uint8_t* d_model_valid, size_t model_valid_pitch, size_t model_valid_stride,
                              uint8_t* d_model_render, size_t model_render_pitch, size_t model_render_stride, uint32_t* d_hole_counts, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_color || !d_mask || !d_valid || !d_render || !d_model_valid || !d_model_render || !d_hole_counts) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (!multiples_of(4, d_hole_counts)) return fail(c, MDVT_ERR_INVALID_ARG, "d_hole_counts must be 4-byte aligned");
    if (eye_w < 1 || eye_h < 1 || model_w < 1 || model_h < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d -> %d x %d", eye_w, eye_h, model_w, model_h);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (eye != 0 && eye != 1) return fail(c, MDVT_ERR_INVALID_ARG, "eye must be 0 (left half) or 1 (right half), got %d", eye);
    if (color_pitch < (size_t)eye_w * 6u || mask_pitch < (size_t)eye_w * 6u) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one side-by-side row");
    if (valid_pitch < (size_t)eye_w || render_pitch < (size_t)eye_w * 3u || model_valid_pitch < (size_t)model_w || model_render_pitch < (size_t)model_w * 3u)
        return fail(c, MDVT_ERR_INVALID_ARG, "output pitch smaller than one row");
    if (n_frames > 1 && (color_stride < color_pitch * (size_t)eye_h || mask_stride < mask_pitch * (size_t)eye_h || valid_stride < valid_pitch * (size_t)eye_h ||
                         render_stride < render_pitch * (size_t)eye_h || model_valid_stride < model_valid_pitch * (size_t)model_h ||
                         model_render_stride < model_render_pitch * (size_t)model_h))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if ((uint64_t)eye_w * (uint64_t)eye_h >= ((uint64_t)1 << 31) || (uint64_t)model_w * (uint64_t)model_h >= ((uint64_t)1 << 31))
        return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large (%d x %d -> %d x %d)", eye_w, eye_h, model_w, model_h);
    if (eye_h > 65535 || model_h > 65535) return fail(c, MDVT_ERR_UNSUPPORTED, "more than 65535 rows (%d, %d)", eye_h, model_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) color_stride = mask_stride = valid_stride = render_stride = model_valid_stride = model_render_stride = 0;
    mdvt::InspatioPrepareArgs a{};
    const size_t at = (size_t)eye * 3u * (size_t)eye_w;
    a.color = {d_color + at, color_pitch, color_stride}; a.mask = {d_mask + at, mask_pitch, mask_stride};
    a.rs = mdvt::adapter_resize(eye_w, eye_h, model_w, model_h);
    a.valid = d_valid; a.valid_pitch = valid_pitch; a.valid_stride = valid_stride;
    a.render = d_render; a.render_pitch = render_pitch; a.render_stride = render_stride;
    a.m_valid = d_model_valid; a.m_valid_pitch = model_valid_pitch; a.m_valid_stride = model_valid_stride;
    a.m_render = d_model_render; a.m_render_pitch = model_render_pitch; a.m_render_stride = model_render_stride;
    a.holes = d_hole_counts;
    MDVT_HIP(c, hipMemsetAsync(d_hole_counts, 0, (size_t)n_frames * sizeof(uint32_t), s));
    for (int f0 = 0; f0 < n_frames; f0 += 32768) {
        a.frame0 = f0;
        MDVT_HIP(c, mdvt::launch_inspatio_prepare(a, set_len(n_frames, f0, 32768), s));
    }
    return MDVT_OK;
}

// No scratch block: launches only.
int mdvt_inspatio_model_frames(mdvt_ctx* c, int in_w, int in_h, int n_frames, const uint8_t* d_frames, size_t frames_pitch, size_t frames_stride,
                               int model_w, int model_h, uint8_t* d_out, size_t out_pitch, size_t out_stride, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_frames || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (in_w < 1 || in_h < 1 || model_w < 1 || model_h < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d -> %d x %d", in_w, in_h, model_w, model_h);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (frames_pitch < (size_t)in_w * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "frames_pitch smaller than one row");
    if (out_pitch < (size_t)model_w * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "out_pitch smaller than one row");
    if (n_frames > 1 && (frames_stride < frames_pitch * (size_t)in_h || out_stride < out_pitch * (size_t)model_h))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if ((uint64_t)in_w * (uint64_t)in_h >= ((uint64_t)1 << 31) || (uint64_t)model_w * (uint64_t)model_h >= ((uint64_t)1 << 31))
        return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large (%d x %d -> %d x %d)", in_w, in_h, model_w, model_h);
    if (model_h > 65535) return fail(c, MDVT_ERR_UNSUPPORTED, "more than 65535 rows (%d)", model_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) frames_stride = out_stride = 0;
    mdvt::InspatioPrepareArgs a{};
    a.color = {d_frames, frames_pitch, frames_stride}; a.mask = {nullptr, 0, 0};
    a.rs = mdvt::adapter_resize(in_w, in_h, model_w, model_h);
    a.m_render = d_out; a.m_render_pitch = out_pitch; a.m_render_stride = out_stride;
    for (int f0 = 0; f0 < n_frames; f0 += 32768) {
        a.frame0 = f0;
        MDVT_HIP(c, mdvt::launch_inspatio_prepare(a, set_len(n_frames, f0, 32768), s));
    }
    return MDVT_OK;
}

// One scratch block (SCR_ADAPTER, as mdvt_adapter_composite_eye): the march's listed-pixel workspace | the marks image | the grown plane.
int mdvt_inspatio_composite_eye(mdvt_ctx* c, int eye_w, int eye_h, int n_frames, int eye,
                                const uint8_t* d_aligned, size_t aligned_pitch, size_t aligned_stride,
                                const uint8_t* d_color, size_t color_pitch, size_t color_stride,
                                const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride,
                                uint8_t* d_pasted, size_t pasted_pitch, size_t pasted_stride,
                                uint8_t* d_blended, size_t blended_pitch, size_t blended_stride, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_aligned || !d_color || !d_mask || !d_pasted) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (eye_w < 1 || eye_h < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d", eye_w, eye_h);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (eye != 0 && eye != 1) return fail(c, MDVT_ERR_INVALID_ARG, "eye must be 0 (left half) or 1 (right half), got %d", eye);
    if (aligned_pitch < (size_t)eye_w * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "aligned_pitch smaller than one row");
    if (color_pitch < (size_t)eye_w * 6u || mask_pitch < (size_t)eye_w * 6u || pasted_pitch < (size_t)eye_w * 6u || (d_blended && blended_pitch < (size_t)eye_w * 6u))
        return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one side-by-side row");
    if (n_frames > 1 && (aligned_stride < aligned_pitch * (size_t)eye_h || color_stride < color_pitch * (size_t)eye_h || mask_stride < mask_pitch * (size_t)eye_h ||
                         pasted_stride < pasted_pitch * (size_t)eye_h || (d_blended && blended_stride < blended_pitch * (size_t)eye_h)))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if (eye_w < 8 || eye_h < 8) return fail(c, MDVT_ERR_UNSUPPORTED, "an eye below 8 x 8 (%d x %d)", eye_w, eye_h);
    if (eye_h > 65535) return fail(c, MDVT_ERR_UNSUPPORTED, "eye too tall (%d rows)", eye_h);
    if (mask_pitch >= (1u << 24) || (unsigned long long)mask_pitch * (unsigned long long)eye_h > 0xFFFFFFFFull)
        return fail(c, MDVT_ERR_UNSUPPORTED, "mask frame too large for the march's 32-bit offsets (pitch %zu, %d rows)", mask_pitch, eye_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t npx = (size_t)eye_w * (size_t)eye_h;
    const size_t ni = (mdvt::normal_infill_workspace_bytes(1, eye_w, eye_h) + 255) & ~(size_t)255;
    uint8_t *ws = nullptr, *marks = nullptr, *grown = nullptr;
    if (d_blended) {
        MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_ADAPTER], ni + 8 * npx, s));       // (the adapter's own size: the two calls share the block)
        ws = c->scratch[SCR_ADAPTER].p; marks = ws + ni; grown = marks + 3 * npx;
    }
    mdvt::InspatioCompositeArgs a{};
    a.W = eye_w; a.H = eye_h; a.aligned_pitch = aligned_pitch; a.color_pitch = color_pitch; a.mask_pitch = mask_pitch;
    a.pasted_pitch = pasted_pitch; a.blended_pitch = blended_pitch; a.grown = grown;
    const size_t at = (size_t)eye * 3u * (size_t)eye_w;
    for (int f = 0; f < n_frames; ++f) {
        const size_t k = n_frames > 1 ? (size_t)f : 0;
        const uint8_t* mask = d_mask + k * mask_stride + at;
        if (d_blended) {
            MDVT_HIP(c, mdvt::launch_mark_lower_side(mask, mask_pitch, marks, (size_t)3 * eye_w, eye_w, eye_h, 30, ws, s));     // iwi:504, 506
            MDVT_HIP(c, mdvt::launch_inspatio_grow(marks, (size_t)3 * eye_w, grown, eye_w, eye_h, s));                          // iwi:505, 507
        }
        a.aligned = d_aligned + k * aligned_stride; a.color = d_color + k * color_stride + at; a.mask = mask;
        a.pasted = d_pasted + k * pasted_stride + at; a.blended = d_blended ? d_blended + k * blended_stride + at : nullptr;
        MDVT_HIP(c, mdvt::launch_inspatio_composite(a, s));
    }
    return MDVT_OK;
}

}  // extern "C"
