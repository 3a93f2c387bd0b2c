// mdvt_api_video_mask.hip -- the three entry points of include/mdvt_video_mask.h: Pillow's 8-bit Lanczos resize, rembg's normalize in
// front of the mask network and its predict's tail behind it (kernels: mdvt_video_mask.hip; the tables: mdvt_lanczos_table.h).  An entry
// point's refusals stand in the order the caller meets their texts, each fail(...) text at its check; the layout tests, set loops
// and the scratch carver are mdvt_context.h's.  Host code only.
#include "mdvt_context.h"
#include "mdvt_video_mask.h"

using namespace mdvt;
using namespace mdvt::host;

namespace {

constexpr size_t kTablePairs = 32;             // pairs the host keeps before it starts over

// One resize as the entry points plan it: which passes run, in which form, and what a frame of a launch set needs for it.
struct ResizePlan {
    int in_w, in_h, out_w, out_h, C;
    bool rows, cols;                           // the horizontal / the vertical pass runs (its sizes differ)
    int form;                                  // MDVT_LANCZOS_FUSED or MDVT_LANCZOS_TWO_LAUNCH; 0: both passes skipped
    size_t tmp_bytes;                          // per frame: the intermediate image of the two-launch form, 0 where none exists
    LzAxis h{}, v{};
};

bool fused_fits(int in_w, int in_h, int out_w, int out_h, int C)
{
    return in_w != out_w && in_h != out_h && (size_t)in_h * (size_t)(kLzStrip * C) <= kLzFusedLds;
}

// The library's choice is the two-launch form: measured, the fused form takes about twice as long at 16 x 1080p and at 8 x 2160p,
// both to 320 x 320 (profiles/r19_video_mask.md).  The fused form runs where a caller asks for it.
ResizePlan plan_resize(int in_w, int in_h, int out_w, int out_h, int C, int form)
{
    ResizePlan p{};
    p.in_w = in_w; p.in_h = in_h; p.out_w = out_w; p.out_h = out_h; p.C = C;
    p.rows = in_w != out_w; p.cols = in_h != out_h;
    if (!p.rows && !p.cols) p.form = 0;
    else if (form) p.form = form;
    else p.form = MDVT_LANCZOS_TWO_LAUNCH;
    p.tmp_bytes = p.form == MDVT_LANCZOS_TWO_LAUNCH && p.rows && p.cols ? up16((size_t)in_h * (size_t)out_w * (size_t)C) : 0;
    return p;
}

const LanczosTable* table_for(mdvt_ctx* c, int in, int out)
{
    auto it = c->lanczos_tables.find({in, out});
    if (it != c->lanczos_tables.end()) return &it->second;
    LanczosTable t;
    if (!build_lanczos_table(in, out, t)) return nullptr;
    return &c->lanczos_tables.emplace(std::make_pair(in, out), std::move(t)).first->second;
}

// The plan's tables onto the device, on the call's stream: built once per (in, out) pair, uploaded when the pairs in
// SCR_LANCZOS_TABLES are others.  The host copies stay where they are while a copy may read them: the map's nodes do not move, and
// it is emptied only after the stream has been waited for.
int stage_tables(mdvt_ctx* c, ResizePlan& p, hipStream_t s)
{
    if (!p.rows && !p.cols) return MDVT_OK;
    if (c->lanczos_tables.size() >= kTablePairs) {
        MDVT_HIP(c, hipStreamSynchronize(s));
        c->lanczos_tables.clear();
    }
    const LanczosTable* th = p.rows ? table_for(c, p.in_w, p.out_w) : nullptr;
    const LanczosTable* tv = p.cols ? table_for(c, p.in_h, p.out_h) : nullptr;
    if ((p.rows && !th) || (p.cols && !tv))
        return fail(c, MDVT_ERR_UNSUPPORTED, "no Lanczos table for %d x %d -> %d x %d", p.in_w, p.in_h, p.out_w, p.out_h);
    const size_t hb = th ? up16(th->bounds.size() * 4) : 0, hc = th ? up16(th->coef.size() * 4) : 0;
    const size_t vb = tv ? up16(tv->bounds.size() * 4) : 0, vc = tv ? up16(tv->coef.size() * 4) : 0;
    bool grew = false;
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_LANCZOS_TABLES], hb + hc + vb + vc, s, &grew));
    uint8_t* w = c->scratch[SCR_LANCZOS_TABLES].p;
    const int want[4] = {p.rows ? p.in_w : 0, p.rows ? p.out_w : 0, p.cols ? p.in_h : 0, p.cols ? p.out_h : 0};
    if (grew || memcmp(want, c->lanczos_resident, sizeof want) != 0) {
        memset(c->lanczos_resident, 0, sizeof c->lanczos_resident);
        if (th) {
            MDVT_HIP(c, hipMemcpyAsync(w, th->bounds.data(), th->bounds.size() * 4, hipMemcpyHostToDevice, s));
            MDVT_HIP(c, hipMemcpyAsync(w + hb, th->coef.data(), th->coef.size() * 4, hipMemcpyHostToDevice, s));
        }
        if (tv) {
            MDVT_HIP(c, hipMemcpyAsync(w + hb + hc, tv->bounds.data(), tv->bounds.size() * 4, hipMemcpyHostToDevice, s));
            MDVT_HIP(c, hipMemcpyAsync(w + hb + hc + vb, tv->coef.data(), tv->coef.size() * 4, hipMemcpyHostToDevice, s));
        }
        memcpy(c->lanczos_resident, want, sizeof want);
    }
    p.h.bounds = reinterpret_cast<const int32_t*>(w); p.h.coef = reinterpret_cast<const int32_t*>(w + hb);
    p.v.bounds = reinterpret_cast<const int32_t*>(w + hb + hc); p.v.coef = reinterpret_cast<const int32_t*>(w + hb + hc + vb);
    return MDVT_OK;
}

struct Image { const uint8_t* p; size_t pitch, stride; };

// n frames (one launch set, at most kGridFrames) of src through the plan to dst; tmp: n * p.tmp_bytes of workspace.
hipError_t resize_set(const ResizePlan& p, Image src, uint8_t* dst, size_t dst_pitch, size_t dst_stride, int rep, uint8_t* tmp, int n, hipStream_t s)
{
    LzArgs a{};
    a.src = src.p; a.src_pitch = src.pitch; a.src_stride = src.stride;
    a.dst = dst; a.dst_pitch = dst_pitch; a.dst_stride = dst_stride;
    a.C = p.C; a.rep = rep; a.in_w = p.in_w; a.in_h = p.in_h; a.out_w = p.out_w; a.out_h = p.out_h; a.h = p.h; a.v = p.v;
    if (p.form == 0) return launch_lz_copy(a, n, s);
    if (p.form == MDVT_LANCZOS_FUSED) return launch_lz_fused(a, n, s);
    if (p.rows && p.cols) {
        LzArgs first = a;                                            // rows: src -> tmp, tight, in_h rows
        first.dst = tmp; first.dst_pitch = (size_t)p.out_w * (size_t)p.C; first.dst_stride = p.tmp_bytes; first.rep = 1;
        hipError_t e = launch_lz_rows(first, n, s);
        if (e != hipSuccess) return e;
        a.src = tmp; a.src_pitch = first.dst_pitch; a.src_stride = first.dst_stride;
        return launch_lz_cols(a, n, s);
    }
    return p.rows ? launch_lz_rows(a, n, s) : launch_lz_cols(a, n, s);
}

// the frames of a launch set: what the workspace budget affords of per_frame bytes each, at most kGridFrames
int set_frames(const mdvt_ctx* c, size_t per_frame, int n_frames)
{
    const int cap = set_len(n_frames, 0, kGridFrames);
    return per_frame ? slots_afforded(c, per_frame, cap) : cap;
}

bool beyond(int a, int b, int c2, int d) { return a > kLanczosMaxSize || b > kLanczosMaxSize || c2 > kLanczosMaxSize || d > kLanczosMaxSize; }

}  // namespace

extern "C" {

// Image.resize((out_w, out_h), LANCZOS).  Launch sets only in the two-launch form with both passes (its intermediate image).
int mdvt_lanczos_resize_u8(mdvt_ctx* c, int in_w, int in_h, int channels, int n_frames, const uint8_t* d_in, size_t in_pitch, size_t in_stride,
                           int out_w, int out_h, uint8_t* d_out, size_t out_pitch, size_t out_stride, int form, int* h_form, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_in || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (in_w < 1 || in_h < 1 || out_w < 1 || out_h < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d -> %d x %d", in_w, in_h, out_w, out_h);
    if (channels != 1 && channels != 3) return fail(c, MDVT_ERR_INVALID_ARG, "channels must be 1 or 3, got %d", channels);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (form < 0 || form > 2) return fail(c, MDVT_ERR_INVALID_ARG, "form must be 0 (the library's choice), 1 (fused) or 2 (two launches), got %d", form);
    if (in_pitch < (size_t)in_w * (size_t)channels) return fail(c, MDVT_ERR_INVALID_ARG, "in_pitch smaller than one row");
    if (out_pitch < (size_t)out_w * (size_t)channels) return fail(c, MDVT_ERR_INVALID_ARG, "out_pitch smaller than one row");
    if (n_frames > 1 && (in_stride < in_pitch * (size_t)in_h || out_stride < out_pitch * (size_t)out_h))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if (beyond(in_w, in_h, out_w, out_h)) return fail(c, MDVT_ERR_UNSUPPORTED, "size beyond 8192 (%d x %d -> %d x %d)", in_w, in_h, out_w, out_h);
    if (form == MDVT_LANCZOS_FUSED && !fused_fits(in_w, in_h, out_w, out_h, channels))
        return fail(c, MDVT_ERR_UNSUPPORTED, "the fused form needs both passes and in_h * %d * channels <= %zu bytes of LDS (%d x %d -> %d x %d)",
                    kLzStrip, kLzFusedLds, in_w, in_h, out_w, out_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) in_stride = out_stride = 0;
    ResizePlan p = plan_resize(in_w, in_h, out_w, out_h, channels, form);
    if (int rc = stage_tables(c, p, s)) return rc;
    const int fchunk = set_frames(c, p.tmp_bytes, n_frames);
    if (p.tmp_bytes) MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_MASK_WS], (size_t)fchunk * p.tmp_bytes, s));
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        const int n = set_len(n_frames, f0, fchunk);
        MDVT_HIP(c, resize_set(p, Image{d_in + (size_t)f0 * in_stride, in_pitch, in_stride}, d_out + (size_t)f0 * out_stride, out_pitch, out_stride, 1,
                               c->scratch[SCR_MASK_WS].p, n, s));
    }
    if (h_form) *h_form = p.form;
    return MDVT_OK;
}

// rembg's normalize.  Launch sets: per frame the resized frame, the two-launch form's intermediate image, the maximum and the table.
int mdvt_mask_model_input(mdvt_ctx* c, int in_w, int in_h, int n_frames, const uint8_t* d_frames, size_t frames_pitch, size_t frames_stride,
                          int order, int model_w, int model_h, const double* h_mean, const double* h_std, float* d_out, size_t out_pitch,
                          size_t out_plane_stride, size_t out_stride, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_frames || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (!h_mean || !h_std) return fail(c, MDVT_ERR_INVALID_ARG, "NULL mean or std");
    if (in_w < 1 || in_h < 1 || model_w < 1 || model_h < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d -> %d x %d", in_w, in_h, model_w, model_h);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (order != 0 && order != 1) return fail(c, MDVT_ERR_INVALID_ARG, "order must be 0 (RGB) or 1 (BGR), got %d", order);
    for (int k = 0; k < 3; ++k)
        if (!(h_mean[k] - h_mean[k] == 0.0) || !(h_std[k] - h_std[k] == 0.0) || h_std[k] == 0.0)
            return fail(c, MDVT_ERR_INVALID_ARG, "mean must be finite, std finite and not 0");
    if (frames_pitch < (size_t)in_w * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "frames_pitch smaller than one row");
    if (out_pitch < (size_t)model_w * 4u) return fail(c, MDVT_ERR_INVALID_ARG, "out_pitch smaller than one row");
    if (out_plane_stride < out_pitch * (size_t)model_h) return fail(c, MDVT_ERR_INVALID_ARG, "out_plane_stride smaller than one plane");
    if (n_frames > 1 && (frames_stride < frames_pitch * (size_t)in_h || out_stride < out_plane_stride * 3u))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if (!multiples_of(4, d_out, out_pitch, out_plane_stride, n_frames > 1 ? out_stride : (size_t)0))
        return fail(c, MDVT_ERR_INVALID_ARG, "d_out, out_pitch and the strides must be multiples of 4");
    if (beyond(in_w, in_h, model_w, model_h)) return fail(c, MDVT_ERR_UNSUPPORTED, "size beyond 8192 (%d x %d -> %d x %d)", in_w, in_h, model_w, model_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) frames_stride = out_stride = 0;
    ResizePlan p = plan_resize(in_w, in_h, model_w, model_h, 3, MDVT_LANCZOS_AUTO);
    if (int rc = stage_tables(c, p, s)) return rc;
    const size_t img_pitch = (size_t)model_w * 3u;
    const size_t img_bytes = p.form ? up16(img_pitch * (size_t)model_h) : 0;      // (equal sizes: the frames themselves are the image)
    const size_t per_frame = p.tmp_bytes + img_bytes + 16 + 768 * sizeof(float);
    const int fchunk = set_frames(c, per_frame, n_frames);
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_MASK_WS], (size_t)fchunk * per_frame, s));
    uint8_t* w = c->scratch[SCR_MASK_WS].p;
    uint8_t* tmp = take<uint8_t>(w, (size_t)fchunk * p.tmp_bytes);
    uint8_t* img = take<uint8_t>(w, (size_t)fchunk * img_bytes);
    MaskInputArgs a{};
    a.lut = take<float>(w, (size_t)fchunk * 768 * sizeof(float));
    a.max_byte = take<uint32_t>(w, (size_t)fchunk * 16);
    a.w = model_w; a.h = model_h; a.bgr = order;
    for (int k = 0; k < 3; ++k) { a.mean[k] = h_mean[k]; a.std[k] = h_std[k]; }
    a.dst_pitch = out_pitch; a.dst_plane = out_plane_stride; a.dst_stride = out_stride;
    a.dst_vec = multiples_of(16, d_out, out_pitch, out_plane_stride, out_stride);
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        const int n = set_len(n_frames, f0, fchunk);
        const Image src{d_frames + (size_t)f0 * frames_stride, frames_pitch, frames_stride};
        if (p.form) {
            MDVT_HIP(c, resize_set(p, src, img, img_pitch, img_bytes, 1, tmp, n, s));
            a.img = img; a.img_pitch = img_pitch; a.img_stride = img_bytes;
        } else {
            a.img = src.p; a.img_pitch = src.pitch; a.img_stride = src.stride;
        }
        a.dst = reinterpret_cast<uint8_t*>(d_out) + (size_t)f0 * out_stride;
        MDVT_HIP(c, launch_mask_model_input(a, n, s));
    }
    return MDVT_OK;
}

// predict's tail and the writer's frame.  Launch sets: per frame the byte plane, the two-launch form's intermediate image, the statistics.
int mdvt_mask_from_prediction(mdvt_ctx* c, int pred_w, int pred_h, int n_frames, const float* d_pred, size_t pred_pitch, size_t pred_stride,
                              int out_w, int out_h, int out_channels, uint8_t* d_mask, size_t mask_pitch, size_t mask_stride, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_pred || !d_mask) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (pred_w < 1 || pred_h < 1 || out_w < 1 || out_h < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d -> %d x %d", pred_w, pred_h, out_w, out_h);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (out_channels != 1 && out_channels != 3) return fail(c, MDVT_ERR_INVALID_ARG, "out_channels must be 1 or 3, got %d", out_channels);
    if (pred_pitch < (size_t)pred_w * 4u) return fail(c, MDVT_ERR_INVALID_ARG, "pred_pitch smaller than one row");
    if (mask_pitch < (size_t)out_w * (size_t)out_channels) return fail(c, MDVT_ERR_INVALID_ARG, "mask_pitch smaller than one row");
    if (n_frames > 1 && (pred_stride < pred_pitch * (size_t)pred_h || mask_stride < mask_pitch * (size_t)out_h))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if (!multiples_of(4, d_pred, pred_pitch, n_frames > 1 ? pred_stride : (size_t)0))
        return fail(c, MDVT_ERR_INVALID_ARG, "d_pred, pred_pitch and pred_stride must be multiples of 4");
    if (beyond(pred_w, pred_h, out_w, out_h)) return fail(c, MDVT_ERR_UNSUPPORTED, "size beyond 8192 (%d x %d -> %d x %d)", pred_w, pred_h, out_w, out_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) pred_stride = mask_stride = 0;
    ResizePlan p = plan_resize(pred_w, pred_h, out_w, out_h, 1, MDVT_LANCZOS_AUTO);
    if (int rc = stage_tables(c, p, s)) return rc;
    const size_t plane_bytes = p.form ? up16((size_t)pred_w * (size_t)pred_h) : 0;           // (equal sizes: the bytes go straight to d_mask)
    const size_t per_frame = p.tmp_bytes + plane_bytes + 16;
    const int fchunk = set_frames(c, per_frame, n_frames);
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_MASK_WS], (size_t)fchunk * per_frame, s));
    uint8_t* w = c->scratch[SCR_MASK_WS].p;
    uint8_t* tmp = take<uint8_t>(w, (size_t)fchunk * p.tmp_bytes);
    uint8_t* plane = take<uint8_t>(w, (size_t)fchunk * plane_bytes);
    MaskPredArgs a{};
    a.stats = take<uint32_t>(w, (size_t)fchunk * 16);
    a.pred_pitch = pred_pitch; a.pred_stride = pred_stride; a.w = pred_w; a.h = pred_h;
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        const int n = set_len(n_frames, f0, fchunk);
        uint8_t* out = d_mask + (size_t)f0 * mask_stride;
        a.pred = reinterpret_cast<const uint8_t*>(d_pred) + (size_t)f0 * pred_stride;
        if (p.form) { a.dst = plane; a.dst_pitch = (size_t)pred_w; a.dst_stride = plane_bytes; a.rep = 1; }
        else { a.dst = out; a.dst_pitch = mask_pitch; a.dst_stride = mask_stride; a.rep = out_channels; }
        MDVT_HIP(c, launch_mask_pred_bytes(a, n, s));
        if (p.form) MDVT_HIP(c, resize_set(p, Image{plane, (size_t)pred_w, plane_bytes}, out, mask_pitch, mask_stride, out_channels, tmp, n, s));
    }
    return MDVT_OK;
}

}  // extern "C"
