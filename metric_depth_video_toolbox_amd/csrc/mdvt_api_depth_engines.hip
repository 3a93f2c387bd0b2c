// mdvt_api_depth_engines.hip -- the three entry points of include/mdvt_depth_engines.h: frames into a model, PromptDA's prompt and
// UniK3D's focal estimate (kernels: mdvt_depth_engines.hip).  An entry point's refusals stand in the order the caller meets their
// texts, each fail(...) text at its check; the layout tests, set loops and the scratch carver are mdvt_context.h's.  Host code only.
#include "mdvt_context.h"
#include "mdvt_depth_engines.h"

using namespace mdvt;
using namespace mdvt::host;

extern "C" {

// Packed frames to a model's planar input.  No scratch block: launches only.
int mdvt_model_frames(mdvt_ctx* c, int in_w, int in_h, int n_frames, const uint8_t* d_frames, size_t frames_pitch, size_t frames_stride,
                      int order, int out_w, int out_h, int format, void* d_out, size_t out_pitch, size_t out_plane_stride,
                      size_t out_stride, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_frames || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (in_w < 1 || in_h < 1 || out_w < 1 || out_h < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d -> %d x %d", in_w, in_h, out_w, out_h);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (order != 0 && order != 1) return fail(c, MDVT_ERR_INVALID_ARG, "order must be 0 (RGB) or 1 (BGR), got %d", order);
    if (format != 0 && format != 1) return fail(c, MDVT_ERR_INVALID_ARG, "format must be 0 (uint8) or 1 (float32), got %d", format);
    const size_t elem = format ? 4u : 1u;
    if (frames_pitch < (size_t)in_w * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "frames_pitch smaller than one row");
    if (out_pitch < (size_t)out_w * elem) return fail(c, MDVT_ERR_INVALID_ARG, "out_pitch smaller than one row");
    if (out_plane_stride < out_pitch * (size_t)out_h) return fail(c, MDVT_ERR_INVALID_ARG, "out_plane_stride smaller than one plane");
    if (n_frames > 1 && (frames_stride < frames_pitch * (size_t)in_h || out_stride < out_plane_stride * 3u))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if (format == 1 && !multiples_of(4, d_out, out_pitch, out_plane_stride, n_frames > 1 ? out_stride : (size_t)0))
        return fail(c, MDVT_ERR_INVALID_ARG, "float32 output: d_out, out_pitch and the strides must be multiples of 4");
    if ((uint64_t)in_w * (uint64_t)in_h >= ((uint64_t)1 << 31) || (uint64_t)out_w * (uint64_t)out_h >= ((uint64_t)1 << 31))
        return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large (%d x %d -> %d x %d)", in_w, in_h, out_w, out_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) frames_stride = out_stride = 0;
    mdvt::ModelFramesArgs a{};
    a.src = d_frames; a.src_pitch = frames_pitch; a.src_stride = frames_stride; a.bgr = order;
    a.src_vec = multiples_of(4, d_frames, frames_pitch, frames_stride);
    a.rs = mdvt::adapter_resize(in_w, in_h, out_w, out_h);
    a.dst = static_cast<uint8_t*>(d_out); a.dst_pitch = out_pitch; a.dst_plane = out_plane_stride; a.dst_stride = out_stride;
    a.as_float = format;
    a.dst_vec = multiples_of(format ? 16 : 4, d_out, out_pitch, out_plane_stride, out_stride);
    a.gw = ((uint32_t)out_w + 3u) / 4u; a.groups = a.gw * (uint32_t)out_h;
    for (int f0 = 0; f0 < n_frames; f0 += kGridFrames) {
        a.frame0 = f0;
        MDVT_HIP(c, mdvt::launch_model_frames(a, set_len(n_frames, f0, kGridFrames), s));
    }
    return MDVT_OK;
}

// Coded depth frames to the low-resolution prompt.  No scratch block: launches only.
int mdvt_depth_prompt(mdvt_ctx* c, int in_w, int in_h, int n_frames, const uint8_t* d_codes, size_t codes_pitch, size_t codes_stride,
                      int order, double max_depth, int out_w, int out_h, float* d_prompt, size_t prompt_pitch, size_t prompt_stride,
                      void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_codes || !d_prompt) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (in_w < 1 || in_h < 1 || out_w < 1 || out_h < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d -> %d x %d", in_w, in_h, out_w, out_h);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (order != 0 && order != 1) return fail(c, MDVT_ERR_INVALID_ARG, "order must be 0 (RGB) or 1 (BGR), got %d", order);
    if (!(max_depth > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "max_depth must be > 0");
    if (codes_pitch < (size_t)in_w * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "codes_pitch smaller than one row");
    if (prompt_pitch < (size_t)out_w * 4u) return fail(c, MDVT_ERR_INVALID_ARG, "prompt_pitch smaller than one row");
    if (n_frames > 1 && (codes_stride < codes_pitch * (size_t)in_h || prompt_stride < prompt_pitch * (size_t)out_h))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if (!multiples_of(4, d_prompt, prompt_pitch, n_frames > 1 ? prompt_stride : (size_t)0))
        return fail(c, MDVT_ERR_INVALID_ARG, "d_prompt, prompt_pitch and prompt_stride must be multiples of 4");
    if ((int64_t)in_w == 2 * (int64_t)out_w && (int64_t)in_h == 2 * (int64_t)out_h)
        return fail(c, MDVT_ERR_UNSUPPORTED, "an exact 2x reduction is OpenCV's area path (%d x %d -> %d x %d)", in_w, in_h, out_w, out_h);
    if ((uint64_t)in_w * (uint64_t)in_h >= ((uint64_t)1 << 31) || (uint64_t)out_w * (uint64_t)out_h >= ((uint64_t)1 << 31))
        return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large (%d x %d -> %d x %d)", in_w, in_h, out_w, out_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) codes_stride = prompt_stride = 0;
    mdvt::DepthPromptArgs a{};
    a.src = d_codes; a.src_pitch = codes_pitch; a.src_stride = codes_stride; a.in_w = in_w; a.in_h = in_h; a.bgr = order;
    a.src_vec = multiples_of(4, d_codes, codes_pitch, codes_stride);
    a.mult = (float)(max_depth / 4228250625.0);                  // max_depth / 255^4 in double, rounded once (dfh:22)
    a.out_w = out_w; a.out_h = out_h; a.resize = in_w != out_w || in_h != out_h;
    a.ratio_x = (double)in_w / (double)out_w; a.ratio_y = (double)in_h / (double)out_h;
    a.dst = reinterpret_cast<uint8_t*>(d_prompt); a.dst_pitch = prompt_pitch; a.dst_stride = prompt_stride;
    a.dst_vec = multiples_of(16, d_prompt, prompt_pitch, prompt_stride);
    a.gw = ((uint32_t)out_w + 3u) / 4u; a.groups = a.gw * (uint32_t)out_h;
    for (int f0 = 0; f0 < n_frames; f0 += kGridFrames) {
        a.frame0 = f0;
        MDVT_HIP(c, mdvt::launch_depth_prompt(a, set_len(n_frames, f0, kGridFrames), s));
    }
    return MDVT_OK;
}

// UniK3D's focal estimate.  Launch sets: as many frames as the ctx's workspace budget affords.
int mdvt_focal_from_points(mdvt_ctx* c, int width, int height, int n_frames, const float* d_points, int layout, size_t points_pitch,
                           size_t points_plane_stride, size_t points_stride, float* d_focal, uint32_t* d_counts, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_points || !d_focal) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (width < 1 || height < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad point map size %d x %d", width, height);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (layout != 0 && layout != 1) return fail(c, MDVT_ERR_INVALID_ARG, "layout must be 0 ([n, 3, H, W]) or 1 ([n, H, W, 3]), got %d", layout);
    if (points_pitch < (size_t)width * (layout ? 12u : 4u)) return fail(c, MDVT_ERR_INVALID_ARG, "points_pitch smaller than one row");
    if (layout == 0 && points_plane_stride < points_pitch * (size_t)height)
        return fail(c, MDVT_ERR_INVALID_ARG, "points_plane_stride smaller than one plane");
    if (n_frames > 1 && points_stride < (layout ? points_pitch * (size_t)height : points_plane_stride * 3u))
        return fail(c, MDVT_ERR_INVALID_ARG, "points_stride smaller than one frame");
    if (!multiples_of(4, d_points, points_pitch, layout ? (size_t)0 : points_plane_stride, n_frames > 1 ? points_stride : (size_t)0))
        return fail(c, MDVT_ERR_INVALID_ARG, "d_points, points_pitch and the strides must be multiples of 4");
    if (!multiples_of(4, d_focal, d_counts))
        return fail(c, MDVT_ERR_INVALID_ARG, "d_focal and d_counts must be 4-byte aligned");
    if (width > (1 << 23) || height > (1 << 23) || (uint64_t)width * (uint64_t)height > ((uint64_t)1 << 28))
        return fail(c, MDVT_ERR_UNSUPPORTED, "point map too large for the focal estimate (%d x %d)", width, height);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) points_stride = 0;
    const uint32_t npx = (uint32_t)width * (uint32_t)height;
    const uint32_t nchunks = (npx + 8191u) / 8192u, nunits = (npx + mdvt::kFocalUnit - 1u) / mdvt::kFocalUnit;
    // per list (a frame has two): the selected values (4 B per point), the chunk sums, the unit counts and offsets, the count
    const size_t compact_stride = ((size_t)npx + 3) & ~(size_t)3;
    const size_t compact_bytes = compact_stride * sizeof(float);
    const size_t sums_bytes = (size_t)nchunks * sizeof(float), unit_bytes = (size_t)nunits * sizeof(uint32_t);
    const size_t per_frame = 2 * (compact_bytes + up16(sums_bytes) + 2 * up16(unit_bytes) + 16);
    const int fchunk = slots_afforded(c, per_frame, n_frames < 4096 ? n_frames : 4096);
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_FOCAL], (size_t)fchunk * per_frame, s));
    mdvt::FocalArgs a{};
    a.pitch = points_pitch; a.stride = points_stride;
    a.chan_bytes = layout ? 4u : points_plane_stride; a.point_bytes = layout ? 12u : 4u;
    a.W = (uint32_t)width; a.npx = npx; a.nunits = nunits; a.nchunks = nchunks;
    a.half_w = (float)((double)width / 2.0); a.half_h = (float)((double)height / 2.0);
    a.compact_stride = compact_stride;
    uint8_t* w = c->scratch[SCR_FOCAL].p;
    a.compact = take<float>(w, (size_t)fchunk * 2 * compact_bytes);
    a.sums = take<float>(w, up16((size_t)fchunk * 2 * sums_bytes));
    a.unit_cnt = take<uint32_t>(w, up16((size_t)fchunk * 2 * unit_bytes));
    a.unit_off = take<uint32_t>(w, up16((size_t)fchunk * 2 * unit_bytes));
    a.totals = take<uint32_t>(w, (size_t)fchunk * 2 * 16);
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        a.n_frames = set_len(n_frames, f0, fchunk);
        a.points = reinterpret_cast<const uint8_t*>(d_points) + (size_t)f0 * points_stride;
        a.focal = d_focal + 2 * (size_t)f0; a.counts = d_counts ? d_counts + 2 * (size_t)f0 : nullptr;
        MDVT_HIP(c, mdvt::launch_focal_from_points(a, s));
    }
    return MDVT_OK;
}

}  // extern "C"
