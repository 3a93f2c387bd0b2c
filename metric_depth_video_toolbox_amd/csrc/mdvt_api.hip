// mdvt_api.hip -- the entry points of the C ABI beside the render (mdvt_api_render.hip) and the context (mdvt_context.hip): include/mdvt.h's formats,
// equirect, blur, infills and both infill-mask completions, then FFV1 in both directions, the convergence depths, the metric alignment, the depth sink, the
// infill adapter and the two further infill engines (a header of include/ each).  An entry point's refusals stand in the order the caller meets their texts,
// each fail(...) text at its check (tests/refusal_cases.py pins texts and order).  Host code only; the kernels are in the other *.hip units.
#include "mdvt_context.h"
#include "mdvt_ffv1_core.h"
#include "mdvt_ffv1_decode.h"
#include "mdvt_ffv1_stream_decode.h"
#include "mdvt_convergence.h"
#include "mdvt_metric_align.h"
#include "mdvt_depth_sink.h"
#include "mdvt_infill_adapter.h"
#include "mdvt_infill_engines.h"

#include <math.h>

using namespace mdvt;
using namespace mdvt::host;
using namespace mdvt::grid8;          // (the grid-independent launchers)

namespace {

// cv2.getGaussianKernel(n, sigma) as published: exp in f64, the weights added from the first on, scaled by 1 / sum; g[n] stays f64 (the caller
// rounds once to f32).  cv2's "sigma = 0" is 0.3 * ((n - 1) * 0.5 - 1) + 0.8, spelled by the caller as its reference spells it.
void gaussian_weights(int n, double sigma, double* g)
{
    double sum = 0.0;
    for (int i = 0; i < n; ++i) { const double x = (double)i - (n - 1) * 0.5; g[i] = exp(-0.5 / (sigma * sigma) * x * x); sum += g[i]; }
    for (int i = 0; i < n; ++i) g[i] *= 1.0 / sum;
}
// cv2.getGaussianKernel(6, 0); the 2-D kernel is the f64 outer product (sr:124-125) rounded to f32 (what filter2D does for an f32 image).
mdvt::BlurKernel masked_blur_kernel()
{
    double g[6];
    gaussian_weights(6, 0.3 * ((6 - 1) * 0.5 - 1.0) + 0.8, g);
    mdvt::BlurKernel K;
    for (int y = 0; y < 6; ++y) for (int x = 0; x < 6; ++x) K.k[6 * y + x] = (float)(g[y] * g[x]);
    return K;
}
constexpr int kTeleaChunk = mdvt::kTeleaMaxImages;      // images per pass (14 B/px of workspace each)
constexpr int kNormalInfillChunk = 16;       // images per launch set
// FFV1's default state transition tables, built once per process
const mdvt::Ffv1StateTables& ffv1_states() { static const mdvt::Ffv1StateTables tab = mdvt::ffv1_default_states(); return tab; }
// (a vector path's multiples_of: the pitch of a single row is never used)
size_t pitch_in_use(size_t pitch, int rows) { return rows == 1 ? 0 : pitch; }

// The n images (frames, when both eyes travel together) from i0 on of a caller's array.
mdvt::ImageSet slice(const uint8_t* base, size_t pitch, size_t stride, int i0, int n, ptrdiff_t eye_offset = 0)
{
    return mdvt::ImageSet{const_cast<uint8_t*>(base) + (size_t)i0 * stride, pitch, stride, eye_offset, n};
}

// the workspace of the listed-pixel stages (normal_infill, infill_using_mask_normals and their single-image kin) for `chunk` images in flight
hipError_t reserve_ni(mdvt_ctx* c, int chunk, hipStream_t s) { return scratch_reserve(c, c->scratch[SCR_NI], mdvt::normal_infill_workspace_bytes(chunk, c->W, c->H), s); }

// What both infill-mask completions refuse before the device is touched.
int check_finish_args(mdvt_ctx* c, const uint8_t* d_seed, const uint8_t* d_seed_right, size_t seed_pitch, const uint8_t* d_out,
                      const uint8_t* d_out_right, size_t out_pitch, int n_frames)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_seed || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if ((d_seed_right == nullptr) != (d_out_right == nullptr)) return fail(c, MDVT_ERR_INVALID_ARG, "right-eye seed and output go together");
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_images must be >= 1");
    if (seed_pitch < (size_t)3 * c->W || out_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (d_seed == d_out || (d_seed_right && d_seed_right == d_out_right)) return fail(c, MDVT_ERR_INVALID_ARG, "d_out may not alias d_seed");
    return MDVT_OK;
}

// The unreached-pixel counts of a pass of nf frames from f0 on into the caller's array: left eyes of all frames, then right eyes.
int copy_remaining(mdvt_ctx* c, uint32_t* d_remaining, const uint32_t* pass, int n_frames, int f0, int nf, int eyes, hipStream_t s)
{
    if (!d_remaining) return MDVT_OK;
    for (int e = 0; e < eyes; ++e)
        MDVT_HIP(c, hipMemcpyAsync(d_remaining + (size_t)e * n_frames + f0, pass + (size_t)e * nf, (size_t)nf * sizeof(uint32_t),
                                   hipMemcpyDeviceToDevice, s));
    return MDVT_OK;
}

// What mdvt_metric_depth_codes (metric) and mdvt_depth_video_codes share: float32 source planes, a factor on the device and a 0 / 1
// flag of their own (scale_shift and style: the factor is required; scale and nan_to_max: it may be null), codes and optional depth
// planes out.  src_pitch_name, flag_name, plane_pitch_name: the caller's argument names for the refusals' texts.  No scratch block:
// launches only.
int depth_codes(mdvt_ctx* c, bool metric, int in_w, int in_h, int n_frames, const float* d_src, size_t src_pitch, size_t src_stride,
                const char* src_pitch_name, const float* d_factor, int flag, const char* flag_name, double max_depth, int out_w, int out_h,
                uint8_t* d_codes, size_t codes_pitch, size_t codes_stride, int order,
                float* d_plane, size_t plane_pitch, size_t plane_stride, const char* plane_pitch_name, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_src || (metric && !d_factor) || !d_codes) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (in_w < 1 || in_h < 1 || out_w < 1 || out_h < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d -> %d x %d", in_w, in_h, out_w, out_h);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (flag != 0 && flag != 1) return fail(c, MDVT_ERR_INVALID_ARG, "%s must be 0 or 1, got %d", flag_name, flag);
    if (order != 0 && order != 1) return fail(c, MDVT_ERR_INVALID_ARG, "order must be 0 (RGB) or 1 (BGR), got %d", order);
    if (!(max_depth > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "max_depth must be > 0");
    if (src_pitch < (size_t)in_w * 4u) return fail(c, MDVT_ERR_INVALID_ARG, "%s smaller than one row", src_pitch_name);
    if (codes_pitch < (size_t)out_w * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "codes_pitch smaller than one row");
    if (d_plane && plane_pitch < (size_t)out_w * 4u) return fail(c, MDVT_ERR_INVALID_ARG, "%s smaller than one row", plane_pitch_name);
    if (n_frames > 1 && (src_stride < src_pitch * (size_t)in_h || codes_stride < codes_pitch * (size_t)out_h ||
                         (d_plane && plane_stride < plane_pitch * (size_t)out_h)))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if ((uint64_t)out_w * (uint64_t)out_h >= ((uint64_t)1 << 31))
        return fail(c, MDVT_ERR_UNSUPPORTED, "output frame too large (%d x %d)", out_w, out_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) src_stride = codes_stride = plane_stride = 0;
    mdvt::DepthCodesArgs a{};
    a.src = reinterpret_cast<const uint8_t*>(d_src); a.src_pitch = src_pitch; a.src_stride = src_stride; a.in_w = in_w; a.in_h = in_h;
    a.src_vec = multiples_of(16, d_src, src_pitch, src_stride);
    a.fmax = (float)max_depth; a.multi = 4228250625.0 / max_depth;
    a.out_w = out_w; a.out_h = out_h; a.resize = in_w != out_w || in_h != out_h;
    a.ratio_x = (double)in_w / (double)out_w; a.ratio_y = (double)in_h / (double)out_h;
    a.codes = d_codes; a.codes_pitch = codes_pitch; a.codes_stride = codes_stride; a.bgr = order;
    a.codes_vec = multiples_of(4, d_codes, codes_pitch, codes_stride);
    a.plane = reinterpret_cast<uint8_t*>(d_plane); a.plane_pitch = plane_pitch; a.plane_stride = plane_stride;
    a.plane_vec = d_plane && multiples_of(16, d_plane, plane_pitch, plane_stride);
    a.gw = ((uint32_t)out_w + 3u) / 4u; a.groups = a.gw * (uint32_t)out_h;
    if (metric) { a.scale_shift = d_factor; a.style = flag; }
    else { a.scale = d_factor; a.nan_to_max = flag; }
    for (int f0 = 0; f0 < n_frames; f0 += kGridFrames) {
        a.frame0 = f0;
        const int n = set_len(n_frames, f0, kGridFrames);
        MDVT_HIP(c, metric ? mdvt::launch_metric_codes(a, n, s) : mdvt::launch_depth_sink(a, n, s));
    }
    return MDVT_OK;
}

}  // namespace

extern "C" {

int mdvt_decode_depth(mdvt_ctx* c, const uint8_t* d_rgb, size_t rgb_pitch, float* d_depth, size_t depth_pitch,
                      double max_depth, double depth_scale, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_rgb || !d_depth) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (rgb_pitch < (size_t)3 * c->W || depth_pitch < (size_t)4 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (!(max_depth > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "max_depth must be > 0");
    DeviceGuard g(c->device);
    MDVT_HIP(c, launch_decode_depth(d_rgb, rgb_pitch, d_depth, depth_pitch, c->W, c->H,
                                    (float)(max_depth / 4228250625.0), (float)depth_scale, (hipStream_t)stream));
    return MDVT_OK;
}

int mdvt_encode_depth(mdvt_ctx* c, const float* d_depth, size_t depth_pitch, uint8_t* d_rgb, size_t rgb_pitch,
                      double max_depth, int bgr, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_rgb || !d_depth) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (rgb_pitch < (size_t)3 * c->W || depth_pitch < (size_t)4 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (!(max_depth > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "max_depth must be > 0");
    DeviceGuard g(c->device);
    MDVT_HIP(c, launch_encode_depth(d_depth, depth_pitch, d_rgb, rgb_pitch, c->W, c->H, max_depth, bgr, (hipStream_t)stream));
    return MDVT_OK;
}

int mdvt_infill_using_normals(mdvt_ctx* c, const uint8_t* d_color, size_t color_pitch, const uint8_t* d_hole,
                              size_t hole_pitch, const float* d_normal, size_t normal_pitch, uint8_t* d_out,
                              size_t out_pitch, int max_steps, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_color || !d_hole || !d_normal || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (d_out == d_color) return fail(c, MDVT_ERR_INVALID_ARG, "d_out may not alias d_color (sources are read from the input image)");
    if (color_pitch < (size_t)3 * c->W || out_pitch < (size_t)3 * c->W || hole_pitch < (size_t)c->W ||
        normal_pitch < (size_t)12 * c->W || normal_pitch % 4 != 0)
        return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (max_steps < 0) return fail(c, MDVT_ERR_INVALID_ARG, "max_steps must be >= 0");
    if (hole_pitch >= (1u << 24) || (unsigned long long)hole_pitch * c->H > 0xFFFFFFFFull)
        return fail(c, MDVT_ERR_UNSUPPORTED, "hole plane too large for the march's 32-bit offsets (pitch %zu, %d rows)", hole_pitch, c->H);
    DeviceGuard g(c->device);
    MDVT_HIP(c, reserve_ni(c, 1, (hipStream_t)stream));
    MDVT_HIP(c, launch_infill_normals(d_color, color_pitch, d_hole, hole_pitch, d_normal, normal_pitch, d_out, out_pitch,
                                      c->W, c->H, max_steps, c->scratch[SCR_NI].p, (hipStream_t)stream));
    return MDVT_OK;
}

int mdvt_mark_lower_side(mdvt_ctx* c, const uint8_t* d_normals_img, size_t img_pitch, uint8_t* d_out, size_t out_pitch,
                         int max_steps, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_normals_img || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (d_out == d_normals_img) return fail(c, MDVT_ERR_INVALID_ARG, "d_out may not alias the input image");
    if (img_pitch < (size_t)3 * c->W || out_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (max_steps < 0) return fail(c, MDVT_ERR_INVALID_ARG, "max_steps must be >= 0");
    if (img_pitch >= (1u << 24) || (unsigned long long)img_pitch * c->H > 0xFFFFFFFFull)
        return fail(c, MDVT_ERR_UNSUPPORTED, "image too large for the march's 32-bit offsets (pitch %zu, %d rows)", img_pitch, c->H);
    DeviceGuard g(c->device);
    MDVT_HIP(c, reserve_ni(c, 1, (hipStream_t)stream));
    MDVT_HIP(c, launch_mark_lower_side(d_normals_img, img_pitch, d_out, out_pitch, c->W, c->H, max_steps, c->scratch[SCR_NI].p, (hipStream_t)stream));
    return MDVT_OK;
}

int mdvt_touchly_depth(mdvt_ctx* c, const float* d_depth, size_t depth_pitch, uint8_t* d_rgb, size_t rgb_pitch,
                       double touchly_max_depth, double touchly_min_depth, int zero_is_far, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_depth || !d_rgb) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (depth_pitch < (size_t)4 * c->W || rgb_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (!(touchly_max_depth > touchly_min_depth)) return fail(c, MDVT_ERR_INVALID_ARG, "touchly_max_depth must exceed touchly_min_depth");
    DeviceGuard g(c->device);
    // NumPy: f32 array (op) python float -> the scalar is rounded to f32 first
    MDVT_HIP(c, launch_touchly_depth(d_depth, depth_pitch, d_rgb, rgb_pitch, c->W, c->H, (float)touchly_max_depth,
                                     (float)touchly_min_depth, (float)(255.0 / (touchly_max_depth - touchly_min_depth)),
                                     zero_is_far, (hipStream_t)stream));
    return MDVT_OK;
}

int mdvt_equirect_tables(int width, int height, double input_fov_deg, float* h_map_x, float* h_map_y)
{
    if (width < 2 || height < 2 || !h_map_x || !h_map_y) return MDVT_ERR_INVALID_ARG;
    if (!(input_fov_deg > 0.0 && input_fov_deg < 180.0)) return MDVT_ERR_INVALID_ARG;
    // f64 throughout, rounded to f32 at the end like map_x.astype(np.float32) (sr:77-78)
    const double pi = 3.141592653589793;
    const double cx = ((double)width - 1.0) / 2.0, cy = ((double)height - 1.0) / 2.0;
    const double half = (input_fov_deg / 2.0) * (pi / 180.0);
    const double fx = cx / tan(half), fy = cy / tan(half);
    for (int x = 0; x < width; ++x) {
        const double theta = ((double)x - cx) / cx * (pi / 2.0);
        h_map_x[x] = fabs(theta) <= half ? (float)(fx * tan(theta) + cx) : -1.0f;
    }
    for (int y = 0; y < height; ++y) {
        const double phi = ((double)y - cy) / cy * (pi / 2.0);
        h_map_y[y] = fabs(phi) <= half ? (float)(fy * tan(phi) + cy) : -1.0f;
    }
    return MDVT_OK;
}

int mdvt_equirect_remap(mdvt_ctx* c, const uint8_t* d_src, size_t src_pitch, size_t src_stride, uint8_t* d_dst,
                        size_t dst_pitch, size_t dst_stride, int n_images, const float* d_map_x, const float* d_map_y,
                        void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_src || !d_dst || !d_map_x || !d_map_y) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (n_images < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_images must be >= 1");
    if (src_pitch < (size_t)3 * c->W || dst_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (d_src == d_dst) return fail(c, MDVT_ERR_INVALID_ARG, "d_dst may not alias d_src");
    DeviceGuard g(c->device);
    MDVT_HIP(c, launch_equirect_remap(d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride, n_images, c->W, c->H,
                                      d_map_x, d_map_y, (hipStream_t)stream));
    return MDVT_OK;
}

int mdvt_swap_rb(mdvt_ctx* c, const uint8_t* d_src, size_t src_pitch, size_t src_stride, uint8_t* d_dst, size_t dst_pitch,
                 size_t dst_stride, int n_images, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_src || !d_dst) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (n_images < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_images must be >= 1");
    if (src_pitch < (size_t)3 * c->W || dst_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    DeviceGuard g(c->device);
    const mdvt::ImageSet in = slice(d_src, src_pitch, src_stride, 0, n_images), out = slice(d_dst, dst_pitch, dst_stride, 0, n_images);
    MDVT_HIP(c, launch_swap_rb(in, out, n_images, c->W, c->H, (hipStream_t)stream));
    return MDVT_OK;
}

int mdvt_masked_blur(mdvt_ctx* c, const uint8_t* d_img, size_t img_pitch, uint8_t* d_out, size_t out_pitch, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_img || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (img_pitch < (size_t)3 * c->W || out_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (d_img == d_out) return fail(c, MDVT_ERR_INVALID_ARG, "d_out may not alias d_img");
    DeviceGuard g(c->device);
    const mdvt::ImageSet in = slice(d_img, img_pitch, 0, 0, 1), out = slice(d_out, out_pitch, 0, 0, 1);
    MDVT_HIP(c, launch_masked_blur(in, nullptr, out, 1, c->W, c->H, masked_blur_kernel(), 0u, (hipStream_t)stream));
    return MDVT_OK;
}

int mdvt_normal_infill(mdvt_ctx* c, const uint8_t* d_img, size_t img_pitch, size_t img_stride, const uint8_t* d_infill_mask,
                       size_t mask_pitch, size_t mask_stride, uint8_t* d_out, size_t out_pitch, size_t out_stride, int n_images,
                       void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_img || !d_infill_mask || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (n_images < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_images must be >= 1");
    if (img_pitch < (size_t)3 * c->W || mask_pitch < (size_t)3 * c->W || out_pitch < (size_t)3 * c->W)
        return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (d_out == d_img || d_out == d_infill_mask) return fail(c, MDVT_ERR_INVALID_ARG, "d_out may not alias an input");
    if (mask_pitch >= (1u << 24) || (unsigned long long)mask_pitch * c->H > 0xFFFFFFFFull || (unsigned long long)c->W * c->H > 0xFFFFFFFFull)
        return fail(c, MDVT_ERR_UNSUPPORTED, "image too large for the marches' 32-bit offsets (pitch %zu, %d x %d)", mask_pitch, c->W, c->H);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const int chunk = n_images < kNormalInfillChunk ? n_images : kNormalInfillChunk;
    MDVT_HIP(c, reserve_ni(c, chunk, s));
    const mdvt::BlurKernel K = masked_blur_kernel();
    for (int i0 = 0; i0 < n_images; i0 += chunk) {
        const int n = n_images - i0 < chunk ? n_images - i0 : chunk;
        MDVT_HIP(c, launch_normal_infill(slice(d_img, img_pitch, img_stride, i0, n), slice(d_infill_mask, mask_pitch, mask_stride, i0, n),
                                         slice(d_out, out_pitch, out_stride, i0, n), c->scratch[SCR_NI].p, n, c->W, c->H, K, s));
    }
    return MDVT_OK;
}

int mdvt_infill_using_mask_normals(mdvt_ctx* c, uint8_t* d_img, size_t img_pitch, size_t img_stride, const uint8_t* d_hole,
                                   size_t hole_pitch, size_t hole_stride, const uint8_t* d_mask_img, size_t mask_pitch,
                                   size_t mask_stride, int n_images, int max_steps, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_img || !d_hole || !d_mask_img) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (n_images < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_images must be >= 1");
    if (img_pitch < (size_t)3 * c->W || mask_pitch < (size_t)3 * c->W || hole_pitch < (size_t)c->W)
        return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (max_steps < 0) return fail(c, MDVT_ERR_INVALID_ARG, "max_steps must be >= 0");
    if (d_img == d_mask_img) return fail(c, MDVT_ERR_INVALID_ARG, "d_img may not alias d_mask_img");
    if (hole_pitch >= (1u << 24) || (unsigned long long)hole_pitch * c->H > 0xFFFFFFFFull)
        return fail(c, MDVT_ERR_UNSUPPORTED, "hole plane too large for the march's 32-bit offsets (pitch %zu, %d rows)", hole_pitch, c->H);
    DeviceGuard g(c->device);
    const int chunk = n_images < kNormalInfillChunk ? n_images : kNormalInfillChunk;
    MDVT_HIP(c, reserve_ni(c, chunk, (hipStream_t)stream));
    for (int i0 = 0; i0 < n_images; i0 += chunk) {
        const int n = n_images - i0 < chunk ? n_images - i0 : chunk;
        MDVT_HIP(c, launch_infill_mask_normals(slice(d_img, img_pitch, img_stride, i0, n), slice(d_hole, hole_pitch, hole_stride, i0, n),
                                               slice(d_mask_img, mask_pitch, mask_stride, i0, n), c->scratch[SCR_NI].p, n, c->W, c->H, max_steps, (hipStream_t)stream));
    }
    return MDVT_OK;
}

static int finish_infill_mask(mdvt_ctx* c, const uint8_t* d_seed, const uint8_t* d_seed_right, size_t seed_pitch, size_t seed_stride,
                              uint8_t* d_out, uint8_t* d_out_right, size_t out_pitch, size_t out_stride, int n_frames, int max_rounds,
                              uint32_t* d_remaining, void* stream)
{
    if (int rc = check_finish_args(c, d_seed, d_seed_right, seed_pitch, d_out, d_out_right, out_pitch, n_frames)) return rc;
    // max_rounds < 0: |max_rounds| levels, every one of them launched without asking the device how many exist (no wait on the stream)
    const bool no_wait = max_rounds < 0;
    if (no_wait) max_rounds = -max_rounds;
    if (max_rounds == 0) max_rounds = 256;
    if (max_rounds > 32766) return fail(c, MDVT_ERR_INVALID_ARG, "max_rounds must be <= 32766");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const int W = c->W, H = c->H;
    const size_t npx = (size_t)W * H;
    if ((unsigned long long)kTeleaChunk * npx > 0xFFFFFFFFull)      // work-list entries are 32-bit pixel indices over a full pass
        return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large for the infill-mask completion (%d x %d)", W, H);
    const int eyes = d_seed_right ? 2 : 1;
    const size_t images = n_frames * eyes < kTeleaChunk ? n_frames * eyes : kTeleaChunk;
    // the per-pixel arrays are sized by the images of a pass, the level counters by max_rounds, the per-image counters hold a full
    // pass; each block keeps the largest size any call has asked of it
    const struct { ScratchId id; size_t bytes; } want[] = {
        {SCR_TELEA_STAMP, images * npx * sizeof(uint16_t)}, {SCR_TELEA_T, images * npx * sizeof(float)},
        {SCR_TELEA_IMG, images * npx * 3 + 4},                       // + 4: pixels are fetched as unaligned dwords
        {SCR_TELEA_NEED, images * npx}, {SCR_TELEA_NLIST, images * npx * sizeof(uint32_t)},
        {SCR_TELEA_COUNTS, mdvt::telea_counter_words(max_rounds) * sizeof(uint32_t)},
        {SCR_TELEA_REMAINING, (size_t)kTeleaChunk * sizeof(uint32_t)}, {SCR_TELEA_LAST_ROUND, (size_t)kTeleaChunk * sizeof(uint32_t)}};
    for (const auto& w : want) MDVT_HIP(c, scratch_reserve(c, c->scratch[w.id], w.bytes, s));
    mdvt::TeleaWorkspace ws{};
    ws.stamp = c->scratch[SCR_TELEA_STAMP].as<uint16_t>(); ws.T = c->scratch[SCR_TELEA_T].as<float>();
    ws.img = c->scratch[SCR_TELEA_IMG].p; ws.need = c->scratch[SCR_TELEA_NEED].p; ws.nlist = c->scratch[SCR_TELEA_NLIST].as<uint32_t>();
    ws.counts = c->scratch[SCR_TELEA_COUNTS].as<uint32_t>();
    ws.offs = ws.counts + (max_rounds + 2);
    ws.ncounts = ws.offs + (max_rounds + 2);
    ws.remaining = c->scratch[SCR_TELEA_REMAINING].as<uint32_t>(); ws.last_round = c->scratch[SCR_TELEA_LAST_ROUND].as<uint32_t>();
    if (!c->telea_levels_host) {
        void *h = nullptr, *d = nullptr;
        size_t got = 0;
        MDVT_HIP(c, pool_take(64, false, -1, &h, &d, &got));          // pinned, from the process-wide pool (see pool_take)
        c->telea_levels_host = (uint32_t*)h;
    }
    const uint32_t key = packed_key_rgb(c);
    const mdvt::BlurKernel K = masked_blur_kernel();
    const int fchunk = kTeleaChunk / eyes;                   // frames per pass: both eyes of a frame travel together
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        const int nf = set_len(n_frames, f0, fchunk), n = nf * eyes;
        const mdvt::ImageSet seed = slice(d_seed, seed_pitch, seed_stride, f0, nf, d_seed_right ? d_seed_right - d_seed : 0);
        const mdvt::ImageSet out = slice(d_out, out_pitch, out_stride, f0, nf, d_out_right ? d_out_right - d_out : 0);
        const mdvt::ImageSet work{ws.img, (size_t)3 * W, 3 * npx, 0, n};
        MDVT_HIP(c, launch_telea_init(seed, ws, n, W, H, max_rounds, key, no_wait ? nullptr : c->telea_levels_host, s));
        MDVT_HIP(c, launch_telea_rounds(ws, W, H, no_wait ? max_rounds : (int)*c->telea_levels_host, key, s));               // sr:806, inpaintRadius = 3
        // (the level lists and T are done with: their storage serves the blur's per-row pixel lists and row counters)
        MDVT_HIP(c, launch_masked_blur(work, &seed, out, n, W, H, K, key, s, ws.nlist, reinterpret_cast<uint32_t*>(ws.T)));   // sr:807-808
        if (int rc = copy_remaining(c, d_remaining, ws.remaining, n_frames, f0, nf, eyes, s)) return rc;
    }
    return MDVT_OK;
}

// The same completion in the heap order of cv2.inpaint (mdvt_telea_heap.hip): one launch per pass, no host read-back.  Images per
// pass: below.
static int finish_infill_mask_heap(mdvt_ctx* c, const uint8_t* d_seed, const uint8_t* d_seed_right, size_t seed_pitch, size_t seed_stride,
                                   uint8_t* d_out, uint8_t* d_out_right, size_t out_pitch, size_t out_stride, int n_frames,
                                   uint32_t* d_remaining, void* stream)
{
    if (int rc = check_finish_args(c, d_seed, d_seed_right, seed_pitch, d_out, d_out_right, out_pitch, n_frames)) return rc;
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const int W = c->W, H = c->H;
    const size_t npx = (size_t)W * H;
    if (npx >= ((size_t)1 << 29))          // activation keys 4 rank + direction and push numbers (< 2 npx) are 32-bit
        return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large for the heap-order completion (%d x %d)", W, H);
    const size_t per_image = mdvt::telea_heap_image_bytes(W, H);
    // images per pass: what fits a quarter of the device's memory and what is free now (the workspace this ctx already holds
    // counts as free: it is reused or handed back first), at most kTeleaHeapMaxImages; both eyes of a frame travel together
    size_t free_b = 0, total_b = 0;
    MDVT_HIP(c, hipMemGetInfo(&free_b, &total_b));
    Scratch& heap = c->scratch[SCR_HEAP_WS];
    const size_t held = heap.bytes;                          // (a whole number of images)
    size_t budget = total_b / 4;
    if (free_b + held < budget) budget = free_b + held;
    size_t cap = budget / per_image;
    if (cap < held / per_image) cap = held / per_image;
    if (cap > (size_t)mdvt::kTeleaHeapMaxImages) cap = mdvt::kTeleaHeapMaxImages;
    const int eyes = d_seed_right ? 2 : 1;
    int fchunk = cap / eyes >= 1 ? (int)(cap / eyes) : 1;                // frames per pass
    const int want_images = (n_frames < fchunk ? n_frames : fchunk) * eyes;
    if (held / per_image < (size_t)want_images) {
        // if the block does not fit after all (another process took the memory meanwhile), fewer images per pass (the old block
        // has gone by then: whatever fits is taken, be it less than before)
        int images = want_images;
        for (;;) {
            const hipError_t e = scratch_reserve(c, heap, (size_t)images * per_image, s);
            if (e == hipSuccess) break;
            (void)hipGetLastError();
            if (images <= eyes)
                return fail(c, MDVT_ERR_OOM, "heap-order completion: no room for the workspace of one %s (%zu bytes): %s",
                            eyes == 2 ? "frame" : "image", (size_t)eyes * per_image, hipGetErrorString(e));
            images = images / 2 / eyes * eyes;
            if (images < eyes) images = eyes;
        }
    }
    const int heap_images = (int)(heap.bytes / per_image);
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_HEAP_REMAINING], (size_t)heap_images * sizeof(uint32_t), s));
    uint32_t* const remaining = c->scratch[SCR_HEAP_REMAINING].as<uint32_t>();
    if (fchunk > heap_images / eyes) fchunk = heap_images / eyes;
    const uint32_t key = packed_key_rgb(c);
    const mdvt::BlurKernel K = masked_blur_kernel();
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        const int nf = set_len(n_frames, f0, fchunk), n = nf * eyes;
        const mdvt::ImageSet seed = slice(d_seed, seed_pitch, seed_stride, f0, nf, d_seed_right ? d_seed_right - d_seed : 0);
        const mdvt::ImageSet out = slice(d_out, out_pitch, out_stride, f0, nf, d_out_right ? d_out_right - d_out : 0);
        const mdvt::ImageSet work{heap.p + mdvt::telea_heap_img_offset(W, H), (size_t)3 * W, per_image, 0, n};
        MDVT_HIP(c, launch_telea_heap(seed, heap.p, per_image, remaining, n, W, H, key, s));     // sr:806, inpaintRadius = 3
        MDVT_HIP(c, launch_masked_blur(work, &seed, out, n, W, H, K, key, s));                                // sr:807-808
        if (int rc = copy_remaining(c, d_remaining, remaining, n_frames, f0, nf, eyes, s)) return rc;
    }
    return MDVT_OK;
}

int mdvt_finish_infill_mask_heap(mdvt_ctx* c, const uint8_t* d_seed, size_t seed_pitch, size_t seed_stride, uint8_t* d_out,
                                 size_t out_pitch, size_t out_stride, int n_images, uint32_t* d_remaining, void* stream)
{
    return finish_infill_mask_heap(c, d_seed, nullptr, seed_pitch, seed_stride, d_out, nullptr, out_pitch, out_stride, n_images,
                                   d_remaining, stream);
}

int mdvt_finish_infill_mask_heap_stereo(mdvt_ctx* c, const uint8_t* d_left_seed, const uint8_t* d_right_seed, size_t seed_pitch,
                                        size_t seed_stride, uint8_t* d_left_out, uint8_t* d_right_out, size_t out_pitch,
                                        size_t out_stride, int n_frames, uint32_t* d_remaining, void* stream)
{
    if (c && (!d_right_seed || !d_right_out)) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    return finish_infill_mask_heap(c, d_left_seed, d_right_seed, seed_pitch, seed_stride, d_left_out, d_right_out, out_pitch,
                                   out_stride, n_frames, d_remaining, stream);
}

int mdvt_finish_infill_mask(mdvt_ctx* c, const uint8_t* d_seed, size_t seed_pitch, size_t seed_stride, uint8_t* d_out,
                            size_t out_pitch, size_t out_stride, int n_images, int max_rounds, uint32_t* d_remaining, void* stream)
{
    return finish_infill_mask(c, d_seed, nullptr, seed_pitch, seed_stride, d_out, nullptr, out_pitch, out_stride, n_images, max_rounds,
                              d_remaining, stream);
}

int mdvt_finish_infill_mask_stereo(mdvt_ctx* c, const uint8_t* d_left_seed, const uint8_t* d_right_seed, size_t seed_pitch,
                                   size_t seed_stride, uint8_t* d_left_out, uint8_t* d_right_out, size_t out_pitch, size_t out_stride,
                                   int n_frames, int max_rounds, uint32_t* d_remaining, void* stream)
{
    if (c && (!d_right_seed || !d_right_out)) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    return finish_infill_mask(c, d_left_seed, d_right_seed, seed_pitch, seed_stride, d_left_out, d_right_out, out_pitch, out_stride,
                              n_frames, max_rounds, d_remaining, stream);
}

// FFV1 packets of device frames (mdvt_ffv1.hip).  Passes: as many frames as the ctx's workspace budget affords, at least one.
int mdvt_encode_video_frames(mdvt_ctx* c, int width, int height, int slices_h, int slices_v, const uint8_t* d_src, size_t pitch,
                            size_t frame_stride, int channels, int order, int n_frames, uint64_t slice_capacity, uint8_t* d_packets,
                            uint64_t packets_cap, uint64_t* d_offsets, uint32_t* d_sizes, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_src || !d_packets || !d_offsets || !d_sizes) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (width < 1 || height < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad frame size %d x %d", width, height);
    if (slices_h < 1 || slices_v < 1 || slices_h > width || slices_v > height || slices_h * slices_v > 1024)
        return fail(c, MDVT_ERR_INVALID_ARG, "bad slice counts %d x %d for %d x %d (each >= 1 and <= the frame's size, product <= 1024)",
                    slices_h, slices_v, width, height);
    if (channels != 1 && channels != 3) return fail(c, MDVT_ERR_INVALID_ARG, "channels must be 1 or 3, got %d", channels);
    if (order != 0 && order != 1) return fail(c, MDVT_ERR_INVALID_ARG, "order must be 0 (RGB) or 1 (BGR), got %d", order);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (pitch < (size_t)width * (size_t)channels) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (n_frames > 1 && frame_stride < pitch * (size_t)height) return fail(c, MDVT_ERR_INVALID_ARG, "frame_stride smaller than one frame");
    if ((uint64_t)width * (uint64_t)height > ((uint64_t)1 << 28))      // (a slice's sample count is a 32-bit word)
        return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large for the device FFV1 encoder (%d x %d)", width, height);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const int spf = slices_h * slices_v;
    // the largest slice: widths and heights of the slices differ by at most one
    const uint64_t max_raw = (uint64_t)((width + slices_h - 1) / slices_h) * (uint64_t)((height + slices_v - 1) / slices_v) * 3u;
    const uint64_t limit = ((uint64_t)1 << 24) - 1;                    // the 24-bit slice size
    const uint64_t want_cap = slice_capacity ? slice_capacity : 2 * max_raw + 4096;
    const uint32_t cap = (uint32_t)(want_cap < limit ? want_cap : limit);
    const size_t slice_stride = ((size_t)cap + 15) & ~(size_t)15;
    const size_t per_frame = (size_t)spf * (slice_stride + sizeof(uint32_t)) + 256;
    const int fchunk = slots_afforded(c, per_frame, n_frames);
    const size_t head = 256;                                           // the running offset, alone on its line
    const size_t words = ((size_t)fchunk * spf * sizeof(uint32_t) + 255) & ~(size_t)255;
    const size_t need = head + words + (size_t)fchunk * spf * slice_stride;
    const Scratch& ws = c->scratch[SCR_FFV1];
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_FFV1], need, s));
    unsigned long long* used = ws.as<unsigned long long>();
    uint32_t* slice_n = reinterpret_cast<uint32_t*>(ws.p + head);
    uint8_t* scratch = ws.p + head + words;
    MDVT_HIP(c, hipMemsetAsync(used, 0, sizeof(unsigned long long), s));
    mdvt::Ffv1CodeArgs ca{};
    ca.pitch = pitch; ca.frame_stride = frame_stride; ca.channels = channels;
    ca.ri = channels == 1 ? 0 : (order == 1 ? 2 : 0); ca.gi = channels == 1 ? 0 : 1; ca.bi = channels == 1 ? 0 : (order == 1 ? 0 : 2);
    ca.W = width; ca.H = height; ca.nh = slices_h; ca.nv = slices_v;
    ca.scratch = scratch; ca.slice_stride = slice_stride; ca.cap = cap; ca.cap_is_24bit = cap == (uint32_t)limit; ca.slice_n = slice_n;
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        const int nf = set_len(n_frames, f0, fchunk);
        ca.src = d_src + (size_t)f0 * frame_stride;
        MDVT_HIP(c, mdvt::launch_ffv1_code(ca, ffv1_states(), nf * spf, s));
        const mdvt::Ffv1LayoutArgs la{slice_n, spf, nf, d_sizes + f0, reinterpret_cast<unsigned long long*>(d_offsets) + f0, used,
                                      (unsigned long long)packets_cap};
        MDVT_HIP(c, mdvt::launch_ffv1_layout(la, s));
        const mdvt::Ffv1EmitArgs ea{slice_n, scratch, slice_stride, spf, d_sizes + f0, reinterpret_cast<unsigned long long*>(d_offsets) + f0,
                                    d_packets};
        MDVT_HIP(c, mdvt::launch_ffv1_emit(ea, nf * spf, s));
    }
    return MDVT_OK;
}

const char* mdvt_ffv1_decode_supported(const uint8_t* h_config, size_t config_size)
{
    mdvt_ffv1::StreamClass sc{};
    return mdvt_ffv1::parse_stream_class(h_config, config_size, false, &sc);
}

const char* mdvt_ffv1_stream_decode_supported(const uint8_t* h_config, size_t config_size)
{
    mdvt_ffv1::StreamClass sc{};
    return mdvt_ffv1::parse_stream_class(h_config, config_size, true, &sc);
}

int mdvt_ffv1_packet_is_key(const uint8_t* h_packet, size_t size)
{
    if (!h_packet || size < 3) return -1;
    return mdvt_ffv1::key_frame_bit(h_packet[0], h_packet[1]);
}

// What both FFV1 decode entry points do before they differ: the argument checks, the record's class (`stream`: the stream
// decoder's, with first_out), the refusals of what the kernels cannot hold, and the fields of `a` that do not depend on the pass.
// n packets, of which those from first_out on are stored.
static int ffv1_decode_prologue(mdvt_ctx* c, bool stream, int width, int height, const uint8_t* h_config, size_t config_size,
                                const uint8_t* d_packets, uint64_t packets_bytes, const uint64_t* d_offsets, const uint32_t* d_sizes, int n,
                                int first_out, uint8_t* d_dst, size_t pitch, size_t frame_stride, int order, uint32_t* d_status,
                                mdvt::Ffv1DecodeArgs* a)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!h_config || !d_packets || !d_offsets || !d_sizes || !d_dst || !d_status) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (width < 1 || height < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad frame size %d x %d", width, height);
    if (order != 0 && order != 1) return fail(c, MDVT_ERR_INVALID_ARG, "order must be 0 (RGB) or 1 (BGR), got %d", order);
    if (n < 1) return fail(c, MDVT_ERR_INVALID_ARG, "%s must be >= 1", stream ? "n_packets" : "n_frames");
    if (first_out < 0 || first_out >= n) return fail(c, MDVT_ERR_INVALID_ARG, "first_out %d outside [0, n_packets = %d)", first_out, n);
    if (pitch < (size_t)width * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (n - first_out > 1 && frame_stride < pitch * (size_t)height) return fail(c, MDVT_ERR_INVALID_ARG, "frame_stride smaller than one frame");
    const char* decoder = stream ? "stream decoder" : "decoder";
    mdvt_ffv1::StreamClass sc{};
    if (const char* why = mdvt_ffv1::parse_stream_class(h_config, config_size, stream, &sc))
        return fail(c, MDVT_ERR_UNSUPPORTED, "FFV1 stream outside the device %s's class: %s", decoder, why);
    if (sc.nh > width || sc.nv > height)
        return fail(c, MDVT_ERR_UNSUPPORTED, "FFV1 stream outside the device %s's class: num_h_slices / num_v_slices %d x %d for a frame of %d x %d",
                    decoder, sc.nh, sc.nv, width, height);
    if ((uint64_t)width * (uint64_t)height > ((uint64_t)1 << 28))
        return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large for the device FFV1 decoder (%d x %d)", width, height);
    // YCbCr: a slice's chroma rectangle starts at (x0 >> hs, y0 >> vs), so the chroma rectangles tile the chroma plane only when
    // every slice origin is a multiple of the subsampling (the host reader's refusal, csrc_host/mdvt_video.cpp check_supported)
    if (sc.planar) {
        for (int sx = 0; sx < sc.nh; ++sx)
            if (((long long)sx * width / sc.nh) & ((1 << sc.hs) - 1))
                return fail(c, MDVT_ERR_UNSUPPORTED, "FFV1 stream outside the device %s's class: num_h_slices / num_v_slices: the %d x %d slice "
                            "grid puts a slice at x = %d of the %d x %d frame, off the chroma grid of shifts (%d, %d)", decoder, sc.nh, sc.nv,
                            (int)((long long)sx * width / sc.nh), width, height, sc.hs, sc.vs);
        for (int sy = 0; sy < sc.nv; ++sy)
            if (((long long)sy * height / sc.nv) & ((1 << sc.vs) - 1))
                return fail(c, MDVT_ERR_UNSUPPORTED, "FFV1 stream outside the device %s's class: num_h_slices / num_v_slices: the %d x %d slice "
                            "grid puts a slice at y = %d of the %d x %d frame, off the chroma grid of shifts (%d, %d)", decoder, sc.nh, sc.nv,
                            (int)((long long)sy * height / sc.nv), width, height, sc.hs, sc.vs);
    }
    const int line_stride = (width + sc.nh - 1) / sc.nh + 2;           // the widest slice, its left and right neighbours
    if (mdvt::ffv1_decode_static_lds_bytes() + mdvt::ffv1_stream_lds_bytes(sc.coder, line_stride) > (size_t)160 * 1024)
        return fail(c, MDVT_ERR_UNSUPPORTED, "a slice of %d pixels' width does not fit the device FFV1 decoder's row buffers (num_h_slices %d)",
                    line_stride - 2, sc.nh);
    a->packets = d_packets; a->packets_bytes = packets_bytes;
    a->W = width; a->H = height; a->nh = sc.nh; a->nv = sc.nv; a->ec = sc.ec; a->coder = sc.coder; a->micro = sc.micro;
    a->pitch = pitch; a->frame_stride = frame_stride; a->ri = order == 1 ? 2 : 0; a->bi = order == 1 ? 0 : 2;
    a->line_stride = line_stride;
    a->planar = sc.planar; a->hs = sc.hs; a->vs = sc.vs;
    return MDVT_OK;
}

// FFV1 packets in device memory -> frames (mdvt_ffv1_decode.hip).  Passes: as many frames as the ctx's workspace budget affords.
int mdvt_decode_video_frames(mdvt_ctx* c, int width, int height, const uint8_t* h_config, size_t config_size, const uint8_t* d_packets,
                             uint64_t packets_bytes, const uint64_t* d_offsets, const uint32_t* d_sizes, int n_frames, uint8_t* d_dst,
                             size_t pitch, size_t frame_stride, int order, uint32_t* d_status, void* stream)
{
    mdvt::Ffv1DecodeArgs a{};                                          // (first_out, kind: none; coder 1)
    if (int e = ffv1_decode_prologue(c, false, width, height, h_config, config_size, d_packets, packets_bytes, d_offsets, d_sizes, n_frames, 0,
                                     d_dst, pitch, frame_stride, order, d_status, &a))
        return e;
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const int spf = a.nh * a.nv;
    const size_t per_frame = (size_t)spf * 3 * sizeof(uint32_t);
    const int fchunk = slots_afforded(c, per_frame, n_frames);
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_FFV1_DEC], (size_t)fchunk * per_frame, s));
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        const int nf = set_len(n_frames, f0, fchunk);
        a.n_frames = nf;
        a.offsets = reinterpret_cast<const unsigned long long*>(d_offsets) + f0; a.sizes = d_sizes + f0;
        a.dst = d_dst + (size_t)f0 * frame_stride; a.status = d_status + f0;
        a.table = c->scratch[SCR_FFV1_DEC].as<uint32_t>();
        a.claims = a.table + (size_t)2 * nf * spf;
        MDVT_HIP(c, hipMemsetAsync(a.claims, 0, (size_t)nf * spf * sizeof(uint32_t), s));
        MDVT_HIP(c, mdvt::launch_ffv1_decode(a, ffv1_states(), s));
    }
    return MDVT_OK;
}

// Consecutive FFV1 packets in device memory -> frames, the context state carried along each key-frame run
// (mdvt_ffv1_stream_decode.hip).  One pass: a run cannot be cut where the workspace budget would cut it.
int mdvt_decode_video_stream(mdvt_ctx* c, int width, int height, const uint8_t* h_config, size_t config_size, const uint8_t* d_packets,
                             uint64_t packets_bytes, const uint64_t* d_offsets, const uint32_t* d_sizes, int n_packets, int first_out,
                             uint8_t* d_dst, size_t pitch, size_t frame_stride, int order, uint32_t* d_status, void* stream)
{
    mdvt::Ffv1DecodeArgs a{};
    if (int e = ffv1_decode_prologue(c, true, width, height, h_config, config_size, d_packets, packets_bytes, d_offsets, d_sizes, n_packets,
                                     first_out, d_dst, pitch, frame_stride, order, d_status, &a))
        return e;
    const int spf = a.nh * a.nv;
    const size_t per_frame = (size_t)spf * 3 * sizeof(uint32_t) + sizeof(uint32_t);
    if (slots_afforded(c, per_frame, n_packets) < n_packets)
        return fail(c, MDVT_ERR_UNSUPPORTED, "%d packets of %d slices pass the workspace budget: split the call at a key frame", n_packets, spf);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_FFV1_STREAM], (size_t)n_packets * per_frame, s));
    a.offsets = reinterpret_cast<const unsigned long long*>(d_offsets); a.sizes = d_sizes;
    a.n_frames = n_packets; a.first_out = first_out;
    a.dst = d_dst; a.status = d_status;
    a.table = c->scratch[SCR_FFV1_STREAM].as<uint32_t>();
    a.claims = a.table + (size_t)2 * n_packets * spf;
    a.kind = a.claims + (size_t)n_packets * spf;
    MDVT_HIP(c, hipMemsetAsync(a.claims, 0, (size_t)n_packets * spf * sizeof(uint32_t), s));
    MDVT_HIP(c, mdvt::launch_ffv1_stream_decode(a, ffv1_states(), s));
    return MDVT_OK;
}

// Per-frame masked depth means (mdvt_convergence.hip).  Launch sets: as many frames as the ctx's workspace budget affords.
int mdvt_convergence_depths(mdvt_ctx* c, int width, int height, const uint8_t* d_depth, size_t depth_pitch, size_t depth_stride, int depth_order,
                            const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride, int mask_order, int n_frames, int n_mask_frames,
                            double max_depth, float* d_means, uint32_t* d_counts, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_depth || !d_means) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (width < 1 || height < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad frame size %d x %d", width, height);
    if (depth_order != 0 && depth_order != 1) return fail(c, MDVT_ERR_INVALID_ARG, "depth_order must be 0 (RGB) or 1 (BGR), got %d", depth_order);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (n_mask_frames < 0 || n_mask_frames > n_frames) return fail(c, MDVT_ERR_INVALID_ARG, "n_mask_frames %d outside [0, n_frames = %d]", n_mask_frames, n_frames);
    if (n_mask_frames > 0 && !d_mask) return fail(c, MDVT_ERR_INVALID_ARG, "n_mask_frames %d without a mask", n_mask_frames);
    if (!(max_depth > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "max_depth must be > 0");
    if (depth_pitch < (size_t)width * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "depth_pitch smaller than one row");
    if (n_frames > 1 && depth_stride < depth_pitch * (size_t)height) return fail(c, MDVT_ERR_INVALID_ARG, "depth_stride smaller than one frame");
    const bool with_mask = d_mask && n_mask_frames > 0;
    if (with_mask) {
        if (mask_order != 0 && mask_order != 1) return fail(c, MDVT_ERR_INVALID_ARG, "mask_order must be 0 (RGB) or 1 (BGR), got %d", mask_order);
        if (mask_pitch < (size_t)width * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "mask_pitch smaller than one row");
        if (n_mask_frames > 1 && mask_stride < mask_pitch * (size_t)height) return fail(c, MDVT_ERR_INVALID_ARG, "mask_stride smaller than one frame");
    }
    if ((uint64_t)width * (uint64_t)height > ((uint64_t)1 << 28))
        return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large for the convergence depths (%d x %d)", width, height);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t npx = (uint32_t)width * (uint32_t)height;
    const uint32_t nchunks = (npx + 8191u) / 8192u, nunits = (npx + 2047u) / 2048u;
    // per frame of a set: the chunk sums; with a mask the ballot words (1 bit/px), the selected codes (2 B/px), unit counts and offsets, the count
    const size_t bits_bytes = with_mask ? (size_t)nunits * 32 * sizeof(unsigned long long) : 0;
    const size_t compact_stride = ((size_t)npx + 7) & ~(size_t)7;
    const size_t compact_bytes = with_mask ? compact_stride * sizeof(uint16_t) : 0;
    const size_t sums_bytes = up16((size_t)nchunks * sizeof(float));
    const size_t unit_bytes = with_mask ? up16((size_t)nunits * sizeof(uint32_t)) : 0;
    const size_t per_frame = bits_bytes + compact_bytes + sums_bytes + 2 * unit_bytes + (with_mask ? 16 : 0);
    const int fchunk = slots_afforded(c, per_frame, n_frames < 4096 ? n_frames : 4096);
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_CONV], (size_t)fchunk * per_frame, s));
    // rows without padding are one long row of npx pixels: no division per pixel, and the 12-byte loads need npx % 4 == 0 only
    const uint32_t depth_W = depth_pitch == (size_t)width * 3u ? npx : (uint32_t)width;
    const uint32_t mask_W = with_mask && mask_pitch == (size_t)width * 3u ? npx : (uint32_t)width;
    mdvt::ConvergenceArgs a{};
    a.depth_pitch = depth_pitch; a.depth_stride = depth_stride; a.depth_bgr = depth_order; a.depth_W = depth_W;
    a.depth_vec = multiples_of(4, d_depth, depth_W, depth_pitch, depth_stride);
    a.mask_pitch = mask_pitch; a.mask_stride = mask_stride; a.mask_bgr = mask_order; a.mask_W = mask_W;
    a.mask_vec = with_mask && multiples_of(4, d_mask, mask_W, mask_pitch, mask_stride);
    a.npx = npx; a.nchunks = nchunks; a.nunits = nunits;
    a.div = (float)(4228250625.0 / max_depth);               // 255^4 / max_depth in double, rounded once (fcd:60)
    a.compact_stride = compact_stride;
    uint8_t* w = c->scratch[SCR_CONV].p;
    a.bits = take<unsigned long long>(w, (size_t)fchunk * bits_bytes);
    a.compact = take<uint16_t>(w, (size_t)fchunk * compact_bytes);
    a.sums = take<float>(w, (size_t)fchunk * sums_bytes);
    a.unit_cnt = take<uint32_t>(w, (size_t)fchunk * unit_bytes);
    a.unit_off = take<uint32_t>(w, (size_t)fchunk * unit_bytes);
    a.totals = take<uint32_t>(w, with_mask ? (size_t)fchunk * 16 : 0);
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        a.n_frames = set_len(n_frames, f0, fchunk);
        a.n_masked = n_mask_frames - f0 < 0 ? 0 : n_mask_frames - f0 < a.n_frames ? n_mask_frames - f0 : a.n_frames;
        a.depth = d_depth + (size_t)f0 * depth_stride;
        a.mask = a.n_masked ? d_mask + (size_t)f0 * mask_stride : nullptr;
        a.means = d_means + f0; a.counts = d_counts ? d_counts + f0 : nullptr;
        MDVT_HIP(c, mdvt::launch_convergence(a, s));
    }
    return MDVT_OK;
}

// The scale-and-shift fit (mdvt_metric_align.hip).  Launch sets of kFitSetChunks chunks; the totals travel in the scratch block.
int mdvt_scale_shift_fit(mdvt_ctx* c, int width, int height, int n_frames, const float* d_pred, size_t pred_pitch, size_t pred_stride,
                         const float* d_target, size_t target_pitch, size_t target_stride, int target_is_depth,
                         const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride, float* d_out, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_pred || !d_target || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (width < 1 || height < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad plane size %d x %d", width, height);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (target_is_depth != 0 && target_is_depth != 1) return fail(c, MDVT_ERR_INVALID_ARG, "target_is_depth must be 0 or 1, got %d", target_is_depth);
    if (pred_pitch < (size_t)width * 4u || target_pitch < (size_t)width * 4u) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (d_mask && mask_pitch < (size_t)width) return fail(c, MDVT_ERR_INVALID_ARG, "mask_pitch smaller than one row");
    if (n_frames > 1 && (pred_stride < pred_pitch * (size_t)height || target_stride < target_pitch * (size_t)height ||
                         (d_mask && mask_stride < mask_pitch * (size_t)height)))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one plane");
    const uint64_t n64 = (uint64_t)n_frames * (uint64_t)width * (uint64_t)height;
    if (n64 >= ((uint64_t)1 << 31)) return fail(c, MDVT_ERR_UNSUPPORTED, "too many values for one fit (%d x %d x %d)", n_frames, width, height);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = (uint32_t)n64, nchunks = (n + 8191u) / 8192u;
    const uint32_t set = nchunks < mdvt::kFitSetChunks ? nchunks : mdvt::kFitSetChunks;
    // 32 B of running totals, then the [5][set] chunk sums of a launch set
    const size_t need = 32 + (size_t)5 * set * sizeof(float);
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_FIT], need, s));
    auto plane = [&](const void* p, size_t pitch, size_t stride, size_t size) {
        mdvt::FitPlane pl{};
        pl.p = static_cast<const uint8_t*>(p); pl.pitch = pitch; pl.stride = n_frames > 1 ? stride : 0; pl.n = n;
        const size_t align = 4 * size;                           // four values
        const bool dense = pitch == (size_t)width * size && (n_frames == 1 || stride == pitch * (size_t)height);
        pl.W = dense ? n : (uint32_t)width;
        pl.HW = dense ? n : (uint32_t)width * (uint32_t)height;
        pl.vec = (uintptr_t)p % align == 0 && (dense || (width % 4 == 0 && pitch % align == 0 && (n_frames == 1 || stride % align == 0)));
        return pl;
    };
    mdvt::FitArgs a{};
    a.pred = plane(d_pred, pred_pitch, pred_stride, 4);
    a.target = plane(d_target, target_pitch, target_stride, 4);
    if (d_mask) a.mask = plane(d_mask, mask_pitch, mask_stride, 1);
    a.target_is_depth = target_is_depth; a.n = n;
    a.state = c->scratch[SCR_FIT].as<float>(); a.sums = a.state + 8; a.sums_stride = set; a.out = d_out;
    for (uint32_t c0 = 0; c0 < nchunks; c0 += mdvt::kFitSetChunks) {
        a.chunk0 = c0;
        a.nchunks_set = nchunks - c0 < mdvt::kFitSetChunks ? nchunks - c0 : mdvt::kFitSetChunks;
        a.first_set = c0 == 0; a.last_set = c0 + a.nchunks_set == nchunks;
        MDVT_HIP(c, mdvt::launch_scale_shift_fit(a, s));
    }
    return MDVT_OK;
}

// Relative planes to metric depth codes (mdvt_metric_align.hip).
int mdvt_metric_depth_codes(mdvt_ctx* c, int in_w, int in_h, int n_frames, const float* d_rel, size_t rel_pitch, size_t rel_stride,
                            const float* d_scale_shift, int style, double max_depth, int out_w, int out_h,
                            uint8_t* d_codes, size_t codes_pitch, size_t codes_stride, int order,
                            float* d_depth, size_t depth_pitch, size_t depth_stride, void* stream)
{
    return depth_codes(c, true, in_w, in_h, n_frames, d_rel, rel_pitch, rel_stride, "rel_pitch", d_scale_shift, style, "style", max_depth, out_w, out_h,
                       d_codes, codes_pitch, codes_stride, order, d_depth, depth_pitch, depth_stride, "depth_pitch", stream);
}

// Metric depth planes to a depth video's codes (mdvt_depth_sink.hip; include/mdvt_depth_sink.h).
int mdvt_depth_video_codes(mdvt_ctx* c, int in_w, int in_h, int n_frames, const float* d_depth, size_t depth_pitch, size_t depth_stride,
                           const float* d_scale, int nan_to_max, double max_depth, int out_w, int out_h,
                           uint8_t* d_codes, size_t codes_pitch, size_t codes_stride, int order,
                           float* d_plane, size_t plane_pitch, size_t plane_stride, void* stream)
{
    return depth_codes(c, false, in_w, in_h, n_frames, d_depth, depth_pitch, depth_stride, "depth_pitch", d_scale, nan_to_max, "nan_to_max", max_depth,
                       out_w, out_h, d_codes, codes_pitch, codes_stride, order, d_plane, plane_pitch, plane_stride, "plane_pitch", stream);
}

}  // extern "C"

// ---- the infill adapter (mdvt_infill_adapter.hip; include/mdvt_infill_adapter.h) ----

namespace {

// cv2.getGaussianKernel(15, 0) as the header restates it: sigma = 0.3 * ((15 - 1) * 0.5 - 1) + 0.8 = 2.6 (the literal); rounded once to f32
mdvt::AdapterGauss adapter_gauss()
{
    double g[15];
    gaussian_weights(15, 2.6, g);
    mdvt::AdapterGauss K;
    for (int i = 0; i < 15; ++i) K.w[i] = (float)g[i];
    return K;
}

// What the two calls on side-by-side frames refuse: the layouts of the colour and mask frames (width 2 * ew) and the sizes.
int check_adapter_sbs(mdvt_ctx* c, int ew, int eh, int n, int eye, const void* d_color, size_t color_pitch, size_t color_stride,
                      const void* d_mask, size_t mask_pitch, size_t mask_stride, int mw, int mh)
{
    if (!d_color || !d_mask) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (ew < 1 || eh < 1 || mw < 1 || mh < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size: eye %d x %d, model %d x %d", ew, eh, mw, mh);
    if (n < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (eye != 0 && eye != 1) return fail(c, MDVT_ERR_INVALID_ARG, "eye must be 0 (left) or 1 (right), got %d", eye);
    if (color_pitch < (size_t)6 * ew || mask_pitch < (size_t)6 * ew) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one side-by-side row");
    if (n > 1 && (color_stride < color_pitch * (size_t)eh || mask_stride < mask_pitch * (size_t)eh))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    return MDVT_OK;
}

}  // namespace

extern "C" {

int mdvt_adapter_prepare_eye(mdvt_ctx* c, int eye_w, int eye_h, int n_frames, int eye,
                             const uint8_t* d_color, size_t color_pitch, size_t color_stride,
                             const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride, int model_w, int model_h,
                             uint8_t* d_image, size_t image_pitch, size_t image_stride,
                             uint8_t* d_model_mask, size_t model_mask_pitch, size_t model_mask_stride, uint32_t* d_hole_counts, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_image || !d_model_mask || !d_hole_counts) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (const int rc = check_adapter_sbs(c, eye_w, eye_h, n_frames, eye, d_color, color_pitch, color_stride, d_mask, mask_pitch, mask_stride, model_w, model_h)) return rc;
    if (image_pitch < (size_t)3 * model_w || model_mask_pitch < (size_t)model_w) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one model row");
    if (n_frames > 1 && (image_stride < image_pitch * (size_t)model_h || model_mask_stride < model_mask_pitch * (size_t)model_h))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one model frame");
    if ((uintptr_t)d_hole_counts % 4) return fail(c, MDVT_ERR_INVALID_ARG, "d_hole_counts must be 4-byte aligned");
    if (model_h > 65535) return fail(c, MDVT_ERR_UNSUPPORTED, "model frame too tall (%d rows)", model_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) color_stride = mask_stride = image_stride = model_mask_stride = 0;
    MDVT_HIP(c, hipMemsetAsync(d_hole_counts, 0, (size_t)n_frames * sizeof(uint32_t), s));
    mdvt::AdapterPrepareArgs a{};
    a.mirror = eye == 0;
    a.rs = mdvt::adapter_resize(eye_w, eye_h, model_w, model_h);
    a.image_pitch = image_pitch; a.image_stride = image_stride; a.mmask_pitch = model_mask_pitch; a.mmask_stride = model_mask_stride;
    for (int f0 = 0; f0 < n_frames; f0 += kGridFrames) {
        a.color = {d_color + (size_t)eye * 3 * eye_w + (size_t)f0 * color_stride, color_pitch, color_stride};
        a.mask = {d_mask + (size_t)eye * 3 * eye_w + (size_t)f0 * mask_stride, mask_pitch, mask_stride};
        a.image = d_image + (size_t)f0 * image_stride; a.mmask = d_model_mask + (size_t)f0 * model_mask_stride; a.holes = d_hole_counts + f0;
        MDVT_HIP(c, mdvt::launch_adapter_prepare(a, set_len(n_frames, f0, kGridFrames), s));
    }
    return MDVT_OK;
}

int mdvt_lhm_moments(mdvt_ctx* c, int width, int height, int n_frames, const uint8_t* d_rgb, size_t pitch, size_t stride,
                     const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride, uint64_t* d_out, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_rgb || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (width < 1 || height < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad frame size %d x %d", width, height);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (pitch < (size_t)3 * width || (d_mask && mask_pitch < (size_t)width)) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (n_frames > 1 && (stride < pitch * (size_t)height || (d_mask && mask_stride < mask_pitch * (size_t)height)))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if ((uintptr_t)d_out % 8) return fail(c, MDVT_ERR_INVALID_ARG, "d_out must be 8-byte aligned");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) stride = mask_stride = 0;
    MDVT_HIP(c, hipMemsetAsync(d_out, 0, (size_t)n_frames * 10 * sizeof(uint64_t), s));
    mdvt::LhmMomentsArgs a{};
    a.W = width; a.H = height;
    a.vec = multiples_of(4, d_rgb, pitch_in_use(pitch, height), stride) && (!d_mask || multiples_of(4, d_mask, pitch_in_use(mask_pitch, height), mask_stride));
    for (int f0 = 0; f0 < n_frames; f0 += kGridFrames) {
        a.img = {d_rgb + (size_t)f0 * stride, pitch, stride};
        a.mask = {d_mask ? d_mask + (size_t)f0 * mask_stride : nullptr, mask_pitch, mask_stride};
        a.out = reinterpret_cast<unsigned long long*>(d_out) + (size_t)f0 * 10;
        MDVT_HIP(c, mdvt::launch_lhm_moments(a, set_len(n_frames, f0, kGridFrames), s));
    }
    return MDVT_OK;
}

int mdvt_lhm_apply(mdvt_ctx* c, int width, int height, int n_frames, const uint8_t* d_rgb, size_t pitch, size_t stride,
                   const double* d_params, uint8_t* d_out, size_t out_pitch, size_t out_stride, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_rgb || !d_params || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (width < 1 || height < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad frame size %d x %d", width, height);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (pitch < (size_t)3 * width || out_pitch < (size_t)3 * width) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (n_frames > 1 && (stride < pitch * (size_t)height || out_stride < out_pitch * (size_t)height))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if ((uintptr_t)d_params % 8) return fail(c, MDVT_ERR_INVALID_ARG, "d_params must be 8-byte aligned");
    if (height > 65535) return fail(c, MDVT_ERR_UNSUPPORTED, "frame too tall (%d rows)", height);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) stride = out_stride = 0;
    mdvt::LhmApplyArgs a{};
    a.W = width; a.H = height; a.out_pitch = out_pitch; a.out_stride = out_stride;
    a.vec = multiples_of(4, d_rgb, pitch_in_use(pitch, height), stride, d_out, pitch_in_use(out_pitch, height), out_stride);
    for (int f0 = 0; f0 < n_frames; f0 += kGridFrames) {
        a.img = {d_rgb + (size_t)f0 * stride, pitch, stride};
        a.params = d_params + (size_t)f0 * 15; a.out = d_out + (size_t)f0 * out_stride;
        MDVT_HIP(c, mdvt::launch_lhm_apply(a, set_len(n_frames, f0, kGridFrames), s));
    }
    return MDVT_OK;
}

int mdvt_adapter_composite_eye(mdvt_ctx* c, int eye_w, int eye_h, int n_frames, int eye,
                               const uint8_t* d_model, int model_w, int model_h, size_t model_pitch, size_t model_stride,
                               const uint8_t* d_color, size_t color_pitch, size_t color_stride,
                               const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride,
                               uint8_t* d_pasted, size_t pasted_pitch, size_t pasted_stride,
                               uint8_t* d_blended, size_t blended_pitch, size_t blended_stride, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_model || !d_pasted || !d_blended) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (const int rc = check_adapter_sbs(c, eye_w, eye_h, n_frames, eye, d_color, color_pitch, color_stride, d_mask, mask_pitch, mask_stride, model_w, model_h)) return rc;
    if (model_pitch < (size_t)3 * model_w) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one model row");
    if (pasted_pitch < (size_t)6 * eye_w || blended_pitch < (size_t)6 * eye_w) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one side-by-side row");
    if (n_frames > 1 && (model_stride < model_pitch * (size_t)model_h || pasted_stride < pasted_pitch * (size_t)eye_h || blended_stride < blended_pitch * (size_t)eye_h))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if (eye_w < 8 || eye_h < 8) return fail(c, MDVT_ERR_UNSUPPORTED, "eye of %d x %d: the 15-tap Gaussian's reflection needs 8 x 8", eye_w, eye_h);
    if (eye_h > 65535) return fail(c, MDVT_ERR_UNSUPPORTED, "eye too tall (%d rows)", eye_h);
    if (mask_pitch >= (1u << 24) || (unsigned long long)mask_pitch * eye_h > 0xFFFFFFFFull)
        return fail(c, MDVT_ERR_UNSUPPORTED, "mask frame too large for the march's 32-bit offsets (pitch %zu, %d rows)", mask_pitch, eye_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    // one frame at a time through: the listed-pixel workspace of the march | the row-blurred plane (f32) | the marks image | the grown plane
    const size_t npx = (size_t)eye_w * eye_h;
    const size_t ni = (mdvt::normal_infill_workspace_bytes(1, eye_w, eye_h) + 255) & ~(size_t)255;
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_ADAPTER], ni + 8 * npx, s));
    uint8_t* const ws = c->scratch[SCR_ADAPTER].p;
    float* const hblur = reinterpret_cast<float*>(ws + ni);
    uint8_t* const marks = ws + ni + 4 * npx;
    uint8_t* const grown = marks + 3 * npx;
    mdvt::AdapterCompositeArgs a{};
    a.mirror = eye == 0;
    a.rs = mdvt::adapter_resize(model_w, model_h, eye_w, eye_h);
    a.grown = grown; a.hblur = hblur; a.pasted_pitch = pasted_pitch; a.blended_pitch = blended_pitch;
    a.g = adapter_gauss();
    const size_t at = (size_t)eye * 3 * eye_w;
    for (int f = 0; f < n_frames; ++f) {
        const size_t k = n_frames > 1 ? (size_t)f : 0;
        const uint8_t* mask = d_mask + k * mask_stride + at;
        MDVT_HIP(c, launch_mark_lower_side(mask, mask_pitch, marks, (size_t)3 * eye_w, eye_w, eye_h, 30, ws, s));           // scr:172-175
        MDVT_HIP(c, mdvt::launch_grow_marks(marks, (size_t)3 * eye_w, grown, eye_w, eye_h, s));                             // scr:177-178
        a.model = {d_model + k * model_stride, model_pitch, 0};
        a.color = {d_color + k * color_stride + at, color_pitch, 0};
        a.mask = {mask, mask_pitch, 0};
        a.pasted = d_pasted + k * pasted_stride + at; a.blended = d_blended + k * blended_stride + at;
        MDVT_HIP(c, mdvt::launch_adapter_composite(a, s));
    }
    return MDVT_OK;
}

// ---- the m2svid and stereo_dissoclusion_net infill steps around their models (include/mdvt_infill_engines.h) ----

int mdvt_m2svid_prepare_eye(mdvt_ctx* c, int eye_w, int eye_h, int n_frames, int eye,
                            const uint8_t* d_color, size_t color_pitch, size_t color_stride,
                            const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride,
                            const uint8_t* d_org, int org_w, int org_h, size_t org_pitch, size_t org_stride,
                            int image_w, int image_h, int mask_w, int mask_h,
                            uint8_t* d_image, size_t image_pitch, size_t image_stride,
                            uint8_t* d_org_image, size_t org_image_pitch, size_t org_image_stride,
                            uint8_t* d_model_mask, size_t model_mask_pitch, size_t model_mask_stride, uint32_t* d_hole_counts, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_org || !d_image || !d_org_image || !d_model_mask || !d_hole_counts) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (const int rc = check_adapter_sbs(c, eye_w, eye_h, n_frames, eye, d_color, color_pitch, color_stride, d_mask, mask_pitch, mask_stride, image_w, image_h)) return rc;
    if (org_w < 1 || org_h < 1 || mask_w < 1 || mask_h < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size: original %d x %d, mask %d x %d", org_w, org_h, mask_w, mask_h);
    if (org_pitch < (size_t)3 * org_w) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row of the original frame");
    if (image_pitch < (size_t)3 * image_w || org_image_pitch < (size_t)3 * image_w || model_mask_pitch < (size_t)mask_w)
        return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one model row");
    if (n_frames > 1 && (org_stride < org_pitch * (size_t)org_h || image_stride < image_pitch * (size_t)image_h ||
                         org_image_stride < org_image_pitch * (size_t)image_h || model_mask_stride < model_mask_pitch * (size_t)mask_h))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if ((uintptr_t)d_hole_counts % 4) return fail(c, MDVT_ERR_INVALID_ARG, "d_hole_counts must be 4-byte aligned");
    if (image_h > 65535 || mask_h > 65535) return fail(c, MDVT_ERR_UNSUPPORTED, "model frame too tall (%d and %d rows)", image_h, mask_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) color_stride = mask_stride = org_stride = image_stride = org_image_stride = model_mask_stride = 0;
    MDVT_HIP(c, hipMemsetAsync(d_hole_counts, 0, (size_t)n_frames * sizeof(uint32_t), s));
    mdvt::M2sPrepareArgs a{};
    a.mirror = eye == 0;
    a.rs_image = mdvt::adapter_resize(eye_w, eye_h, image_w, image_h);
    a.rs_org = mdvt::adapter_resize(org_w, org_h, image_w, image_h);
    a.rs_mask = mdvt::adapter_resize(eye_w, eye_h, mask_w, mask_h);
    a.image_pitch = image_pitch; a.image_stride = image_stride; a.org_image_pitch = org_image_pitch; a.org_image_stride = org_image_stride;
    a.mmask_pitch = model_mask_pitch; a.mmask_stride = model_mask_stride;
    const size_t at = (size_t)eye * 3 * eye_w;
    for (int f0 = 0; f0 < n_frames; f0 += mdvt::kM2sPrepareFrames) {
        a.color = {d_color + at + (size_t)f0 * color_stride, color_pitch, color_stride};
        a.mask = {d_mask + at + (size_t)f0 * mask_stride, mask_pitch, mask_stride};
        a.org = {d_org + (size_t)f0 * org_stride, org_pitch, org_stride};
        a.image = d_image + (size_t)f0 * image_stride; a.org_image = d_org_image + (size_t)f0 * org_image_stride;
        a.mmask = d_model_mask + (size_t)f0 * model_mask_stride; a.holes = d_hole_counts + f0;
        MDVT_HIP(c, mdvt::launch_m2s_prepare(a, n_frames - f0 < mdvt::kM2sPrepareFrames ? n_frames - f0 : mdvt::kM2sPrepareFrames, s));
    }
    return MDVT_OK;
}

int mdvt_model_infill_finish(mdvt_ctx* c, int width, int height, int n_images,
                             const uint8_t* d_img, size_t img_pitch, size_t img_stride,
                             const uint8_t* d_model, size_t model_pitch, size_t model_stride,
                             const uint8_t* d_infill_mask, size_t mask_pitch, size_t mask_stride,
                             uint8_t* d_out, size_t out_pitch, size_t out_stride, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_img || !d_model || !d_infill_mask || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (width < 1 || height < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad image size %d x %d", width, height);
    if (n_images < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_images must be >= 1");
    const size_t row = (size_t)3 * width;
    if (img_pitch < row || model_pitch < row || mask_pitch < row || out_pitch < row) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (n_images > 1 && (img_stride < img_pitch * (size_t)height || model_stride < model_pitch * (size_t)height ||
                         mask_stride < mask_pitch * (size_t)height || out_stride < out_pitch * (size_t)height))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one image");
    if (d_out == d_img || d_out == d_model || d_out == d_infill_mask) return fail(c, MDVT_ERR_INVALID_ARG, "d_out may not alias an input");
    if (mask_pitch >= (1u << 24) || (unsigned long long)mask_pitch * height > 0xFFFFFFFFull)
        return fail(c, MDVT_ERR_UNSUPPORTED, "image too large for the march's 32-bit offsets (pitch %zu, %d x %d)", mask_pitch, width, height);
    if (height > 65535) return fail(c, MDVT_ERR_UNSUPPORTED, "image too tall (%d rows)", height);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_images == 1) img_stride = model_stride = mask_stride = out_stride = 0;
    const int chunk = n_images < kNormalInfillChunk ? n_images : kNormalInfillChunk;
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_NI], mdvt::normal_infill_workspace_bytes(chunk, width, height), s));
    const mdvt::BlurKernel K = masked_blur_kernel();
    for (int i0 = 0; i0 < n_images; i0 += chunk) {
        const int n = n_images - i0 < chunk ? n_images - i0 : chunk;
        MDVT_HIP(c, launch_model_infill_finish(slice(d_img, img_pitch, img_stride, i0, n), slice(d_model, model_pitch, model_stride, i0, n),
                                               slice(d_infill_mask, mask_pitch, mask_stride, i0, n), slice(d_out, out_pitch, out_stride, i0, n),
                                               c->scratch[SCR_NI].p, n, width, height, K, s));
    }
    return MDVT_OK;
}

}  // extern "C"
