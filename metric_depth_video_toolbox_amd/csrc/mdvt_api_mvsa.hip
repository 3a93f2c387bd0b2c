// mdvt_api_mvsa.hip -- the three entry points of include/mdvt_mvsa.h: torch's bilinear resize into the multi-view model, two nearest
// resizes to a depth video's codes and the masked median ratio (kernels: mdvt_mvsa.hip).  An entry point's refusals stand in the
// order the caller meets their texts, each fail(...) text at its check; the layout tests, set loops and the scratch carver are
// mdvt_context.h's.  Host code only.
#include "mdvt_context.h"
#include "mdvt_mvsa.h"

using namespace mdvt;
using namespace mdvt::host;

namespace {

// fl(float(n_in) / float(n_out)): the scale of torch's resizes without a scale factor
inline float size_ratio(int n_in, int n_out) { return (float)n_in / (float)n_out; }

}  // namespace

extern "C" {

// Packed frames to the model's planar float32 input through torch's bilinear resize.  No scratch block: launches only.
int mdvt_bilinear_model_frames(mdvt_ctx* c, int in_w, int in_h, int n_frames, const uint8_t* d_frames, size_t frames_pitch,
                               size_t frames_stride, int order, int out_w, int out_h, float* d_out, size_t out_pitch,
                               size_t out_plane_stride, size_t out_stride, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_frames || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (in_w < 1 || in_h < 1 || out_w < 1 || out_h < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d -> %d x %d", in_w, in_h, out_w, out_h);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (order != 0 && order != 1) return fail(c, MDVT_ERR_INVALID_ARG, "order must be 0 (RGB) or 1 (BGR), got %d", order);
    if (frames_pitch < (size_t)in_w * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "frames_pitch smaller than one row");
    if (out_pitch < (size_t)out_w * 4u) return fail(c, MDVT_ERR_INVALID_ARG, "out_pitch smaller than one row");
    if (out_plane_stride < out_pitch * (size_t)out_h) return fail(c, MDVT_ERR_INVALID_ARG, "out_plane_stride smaller than one plane");
    if (n_frames > 1 && (frames_stride < frames_pitch * (size_t)in_h || out_stride < out_plane_stride * 3u))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if (!multiples_of(4, d_out, out_pitch, out_plane_stride, n_frames > 1 ? out_stride : (size_t)0))
        return fail(c, MDVT_ERR_INVALID_ARG, "d_out, out_pitch and the strides must be multiples of 4");
    if ((uint64_t)in_w * (uint64_t)in_h >= ((uint64_t)1 << 31) || (uint64_t)out_w * (uint64_t)out_h >= ((uint64_t)1 << 31))
        return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large (%d x %d -> %d x %d)", in_w, in_h, out_w, out_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) frames_stride = out_stride = 0;
    mdvt::BilinearFramesArgs a{};
    a.src = d_frames; a.src_pitch = frames_pitch; a.src_stride = frames_stride; a.in_w = in_w; a.in_h = in_h; a.bgr = order;
    a.scale_x = size_ratio(in_w, out_w); a.scale_y = size_ratio(in_h, out_h);
    a.small = (int64_t)out_w + (int64_t)out_h <= 128;             // torch's own choice between its two CPU kernels (include/mdvt_mvsa.h)
    a.dst = reinterpret_cast<uint8_t*>(d_out); a.dst_pitch = out_pitch; a.dst_plane = out_plane_stride; a.dst_stride = out_stride;
    a.out_w = out_w; a.dst_vec = multiples_of(16, d_out, out_pitch, out_plane_stride, out_stride);
    a.gw = ((uint32_t)out_w + 3u) / 4u; a.groups = a.gw * (uint32_t)out_h;
    for (int f0 = 0; f0 < n_frames; f0 += kGridFrames) {
        a.frame0 = f0;
        MDVT_HIP(c, mdvt::launch_bilinear_frames(a, set_len(n_frames, f0, kGridFrames), s));
    }
    return MDVT_OK;
}

// The refined depth through two nearest resizes to codes.  No scratch block: launches only.
int mdvt_nearest_depth_codes(mdvt_ctx* c, int in_w, int in_h, int n_frames, const float* d_depth, size_t depth_pitch, size_t depth_stride,
                             int mid_w, int mid_h, const float* d_scale, size_t scale_stride, double max_depth, int out_w, int out_h,
                             uint8_t* d_codes, size_t codes_pitch, size_t codes_stride, int order,
                             float* d_plane, size_t plane_pitch, size_t plane_stride, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_depth || !d_codes) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (in_w < 1 || in_h < 1 || mid_w < 1 || mid_h < 1 || out_w < 1 || out_h < 1)
        return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d -> %d x %d -> %d x %d", in_w, in_h, mid_w, mid_h, out_w, out_h);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (order != 0 && order != 1) return fail(c, MDVT_ERR_INVALID_ARG, "order must be 0 (RGB) or 1 (BGR), got %d", order);
    if (!(max_depth > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "max_depth must be > 0");
    if (depth_pitch < (size_t)in_w * 4u) return fail(c, MDVT_ERR_INVALID_ARG, "depth_pitch smaller than one row");
    if (codes_pitch < (size_t)out_w * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "codes_pitch smaller than one row");
    if (d_plane && plane_pitch < (size_t)out_w * 4u) return fail(c, MDVT_ERR_INVALID_ARG, "plane_pitch smaller than one row");
    if (n_frames > 1 && (depth_stride < depth_pitch * (size_t)in_h || codes_stride < codes_pitch * (size_t)out_h ||
                         (d_plane && plane_stride < plane_pitch * (size_t)out_h)))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if (!multiples_of(4, d_depth, depth_pitch, n_frames > 1 ? depth_stride : (size_t)0) ||
        (d_plane && !multiples_of(4, d_plane, plane_pitch, n_frames > 1 ? plane_stride : (size_t)0)))
        return fail(c, MDVT_ERR_INVALID_ARG, "float32 planes: pointers, pitches and strides must be multiples of 4");
    if (d_scale && !multiples_of(4, d_scale, n_frames > 1 ? scale_stride : (size_t)0))
        return fail(c, MDVT_ERR_INVALID_ARG, "d_scale and scale_stride must be multiples of 4");
    if ((uint64_t)out_w * (uint64_t)out_h >= ((uint64_t)1 << 31))
        return fail(c, MDVT_ERR_UNSUPPORTED, "output frame too large (%d x %d)", out_w, out_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) depth_stride = codes_stride = plane_stride = scale_stride = 0;
    mdvt::NearestCodesArgs a{};
    a.c.src = reinterpret_cast<const uint8_t*>(d_depth); a.c.src_pitch = depth_pitch; a.c.src_stride = depth_stride; a.c.in_w = in_w; a.c.in_h = in_h;
    a.c.fmax = (float)max_depth; a.c.multi = 4228250625.0 / max_depth;
    a.c.out_w = out_w; a.c.out_h = out_h;
    a.c.codes = d_codes; a.c.codes_pitch = codes_pitch; a.c.codes_stride = codes_stride; a.c.bgr = order;
    a.c.codes_vec = multiples_of(4, d_codes, codes_pitch, codes_stride);
    a.c.plane = reinterpret_cast<uint8_t*>(d_plane); a.c.plane_pitch = plane_pitch; a.c.plane_stride = plane_stride;
    a.c.plane_vec = d_plane && multiples_of(16, d_plane, plane_pitch, plane_stride);
    a.c.gw = ((uint32_t)out_w + 3u) / 4u; a.c.groups = a.c.gw * (uint32_t)out_h;
    a.x = mdvt::NearAxis{size_ratio(mid_w, out_w), size_ratio(in_w, mid_w), mid_w, in_w};
    a.y = mdvt::NearAxis{size_ratio(mid_h, out_h), size_ratio(in_h, mid_h), mid_h, in_h};
    a.scales = reinterpret_cast<const uint8_t*>(d_scale); a.scales_stride = scale_stride;
    for (int f0 = 0; f0 < n_frames; f0 += kGridFrames) {
        a.c.frame0 = f0;
        MDVT_HIP(c, mdvt::launch_nearest_codes(a, set_len(n_frames, f0, kGridFrames), s));
    }
    return MDVT_OK;
}

// The masked median ratio.  Launch sets: as many frames as the ctx's workspace budget affords.
int mdvt_ratio_median(mdvt_ctx* c, int n_frames, int cv_w, int cv_h, const float* d_cv, size_t cv_pitch, size_t cv_stride,
                      int ref_w, int ref_h, const float* d_ref, size_t ref_pitch, size_t ref_stride,
                      int mask_w, int mask_h, const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride,
                      float* d_median, uint32_t* d_counts, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_cv || !d_ref || !d_median) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (cv_w < 1 || cv_h < 1 || ref_w < 1 || ref_h < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d, %d x %d", cv_w, cv_h, ref_w, ref_h);
    if (d_mask && (mask_w < 1 || mask_h < 1)) return fail(c, MDVT_ERR_INVALID_ARG, "bad mask size %d x %d", mask_w, mask_h);
    if (cv_pitch < (size_t)cv_w * 4u) return fail(c, MDVT_ERR_INVALID_ARG, "cv_pitch smaller than one row");
    if (ref_pitch < (size_t)ref_w * 4u) return fail(c, MDVT_ERR_INVALID_ARG, "ref_pitch smaller than one row");
    if (d_mask && mask_pitch < (size_t)mask_w) return fail(c, MDVT_ERR_INVALID_ARG, "mask_pitch smaller than one row");
    if (n_frames > 1 && (cv_stride < cv_pitch * (size_t)cv_h || ref_stride < ref_pitch * (size_t)ref_h ||
                         (d_mask && mask_stride < mask_pitch * (size_t)mask_h)))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if (!multiples_of(4, d_cv, cv_pitch, d_ref, ref_pitch, n_frames > 1 ? cv_stride : (size_t)0, n_frames > 1 ? ref_stride : (size_t)0))
        return fail(c, MDVT_ERR_INVALID_ARG, "float32 planes: pointers, pitches and strides must be multiples of 4");
    if (!multiples_of(4, d_median, d_counts)) return fail(c, MDVT_ERR_INVALID_ARG, "d_median and d_counts must be 4-byte aligned");
    if ((uint64_t)cv_w * (uint64_t)cv_h >= ((uint64_t)1 << 31))
        return fail(c, MDVT_ERR_UNSUPPORTED, "cost volume too large (%d x %d)", cv_w, cv_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) cv_stride = ref_stride = mask_stride = 0;
    const size_t per_frame = (size_t)mdvt::kMedianFrameWords * sizeof(uint32_t);
    const int fchunk = slots_afforded(c, per_frame, n_frames < 4096 ? n_frames : 4096);
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_MVSA], (size_t)fchunk * per_frame, s));
    mdvt::RatioMedianArgs a{};
    a.cv_pitch = cv_pitch; a.cv_stride = cv_stride; a.cv_w = (uint32_t)cv_w; a.npx = (uint32_t)cv_w * (uint32_t)cv_h;
    a.ref_pitch = ref_pitch; a.ref_stride = ref_stride; a.ref_w = ref_w; a.ref_h = ref_h;
    a.ref_sx = size_ratio(ref_w, cv_w); a.ref_sy = size_ratio(ref_h, cv_h);
    if (d_mask) {
        a.mask_pitch = mask_pitch; a.mask_stride = mask_stride; a.mask_w = mask_w; a.mask_h = mask_h;
        a.mask_sx = size_ratio(mask_w, cv_w); a.mask_sy = size_ratio(mask_h, cv_h);
    }
    a.work = c->scratch[SCR_MVSA].as<uint32_t>();
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        a.n_frames = set_len(n_frames, f0, fchunk);
        a.cv = reinterpret_cast<const uint8_t*>(d_cv) + (size_t)f0 * cv_stride;
        a.ref = reinterpret_cast<const uint8_t*>(d_ref) + (size_t)f0 * ref_stride;
        a.mask = d_mask ? d_mask + (size_t)f0 * mask_stride : nullptr;
        a.median = d_median + f0; a.counts = d_counts ? d_counts + f0 : nullptr;
        MDVT_HIP(c, mdvt::launch_ratio_median(a, s));
    }
    return MDVT_OK;
}

}  // extern "C"
