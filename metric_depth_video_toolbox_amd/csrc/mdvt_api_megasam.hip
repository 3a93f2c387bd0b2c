// mdvt_api_megasam.hip -- the entry points of include/mdvt_megasam.h: cv2's area resize, torch's nearest-exact and bilinear resizes into
// the camera tracker and its planes out to video frames (kernels: mdvt_megasam.hip; the tables: mdvt_area_table.h).  An entry point's
// refusals stand in the order the caller meets their texts, each fail(...) text at its check; the layout tests, set loops and the
// scratch carver are mdvt_context.h's.  Host code only.
#include "mdvt_context.h"
#include "mdvt_megasam.h"

using namespace mdvt;
using namespace mdvt::host;

namespace {

constexpr size_t kTablePairs = 32;             // pairs the host keeps before it starts over

// fl(float(n_in) / float(n_out)): the scale of torch's resizes without a scale factor
inline float size_ratio(int n_in, int n_out) { return (float)n_in / (float)n_out; }

const AreaTable* table_for(mdvt_ctx* c, int in, int out)
{
    auto it = c->area_tables.find({in, out});
    if (it != c->area_tables.end()) return &it->second;
    AreaTable t;
    if (!build_area_table(in, out, t)) return nullptr;
    return &c->area_tables.emplace(std::make_pair(in, out), std::move(t)).first->second;
}

// Both axes' tables onto the device, on the call's stream: built once per (in, out) pair, uploaded when the pairs in SCR_AREA_TABLES
// are others (the rule of mdvt_api_video_mask.hip's stage_tables: the map's nodes do not move while a copy may read them, and the map
// is emptied only after the stream has been waited for).
int stage_tables(mdvt_ctx* c, int in_w, int mid_w, int in_h, int mid_h, const AreaTable*& th, const AreaTable*& tv, AreaAxis& x, AreaAxis& y, hipStream_t s)
{
    if (c->area_tables.size() >= kTablePairs) {
        MDVT_HIP(c, hipStreamSynchronize(s));
        c->area_tables.clear();
    }
    th = table_for(c, in_w, mid_w);
    tv = table_for(c, in_h, mid_h);
    if (!th || !tv) return fail(c, MDVT_ERR_UNSUPPORTED, "no area table for %d x %d -> %d x %d", in_w, in_h, mid_w, mid_h);
    const size_t part[6] = {up16(th->first.size() * 4), up16(th->count.size() * 4), up16(th->w.size() * 4),
                            up16(tv->first.size() * 4), up16(tv->count.size() * 4), up16(tv->w.size() * 4)};
    const void* from[6] = {th->first.data(), th->count.data(), th->w.data(), tv->first.data(), tv->count.data(), tv->w.data()};
    const size_t bytes[6] = {th->first.size() * 4, th->count.size() * 4, th->w.size() * 4, tv->first.size() * 4, tv->count.size() * 4, tv->w.size() * 4};
    size_t total = 0;
    for (size_t b : part) total += b;
    bool grew = false;
    MDVT_HIP(c, scratch_reserve(c, c->scratch[SCR_AREA_TABLES], total, s, &grew));
    uint8_t* w = c->scratch[SCR_AREA_TABLES].p;
    uint8_t* at[6];
    for (int k = 0; k < 6; ++k) at[k] = take<uint8_t>(w, part[k]);
    const int want[4] = {in_w, mid_w, in_h, mid_h};
    if (grew || memcmp(want, c->area_resident, sizeof want) != 0) {
        memset(c->area_resident, 0, sizeof c->area_resident);
        for (int k = 0; k < 6; ++k) MDVT_HIP(c, hipMemcpyAsync(at[k], from[k], bytes[k], hipMemcpyHostToDevice, s));
        memcpy(c->area_resident, want, sizeof want);
    }
    x = AreaAxis{reinterpret_cast<const int32_t*>(at[0]), reinterpret_cast<const int32_t*>(at[1]), reinterpret_cast<const float*>(at[2]), th->ktaps};
    y = AreaAxis{reinterpret_cast<const int32_t*>(at[3]), reinterpret_cast<const int32_t*>(at[4]), reinterpret_cast<const float*>(at[5]), tv->ktaps};
    return MDVT_OK;
}

// the bytes a staged source row of the widest tile of tile_w output columns takes in LDS, as k_area_frames lays it out
uint32_t staged_row_bytes(const AreaTable& th, int out_w, int tile_w, bool vec)
{
    uint32_t most = 0;
    for (int x0 = 0; x0 < out_w; x0 += tile_w) {
        const int x1 = (x0 + tile_w < out_w ? x0 + tile_w : out_w) - 1;
        const uint32_t b0 = 3u * (uint32_t)th.first[(size_t)x0], b1 = 3u * (uint32_t)(th.first[(size_t)x1] + th.count[(size_t)x1]);
        const uint32_t span = b1 - (vec ? (b0 & ~15u) : b0);
        if (span > most) most = span;
    }
    return (uint32_t)up16(most);
}

bool whole_ratio(int in, int out) { return in % out == 0; }

// what the three calls that take packed frames refuse alike, in the order of their texts
int check_frames_in(mdvt_ctx* c, int in_w, int in_h, int n_frames, const void* d_frames, size_t frames_pitch, size_t frames_stride, int bgr,
                    int mid_w, int mid_h, int out_w, int out_h, const void* d_out)
{
    if (!d_frames || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (in_w < 1 || in_h < 1 || mid_w < 1 || mid_h < 1 || out_w < 1 || out_h < 1)
        return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d -> %d x %d -> %d x %d", in_w, in_h, mid_w, mid_h, out_w, out_h);
    if (out_w > mid_w || out_h > mid_h) return fail(c, MDVT_ERR_INVALID_ARG, "the crop %d x %d is larger than the resized image %d x %d", out_w, out_h, mid_w, mid_h);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (bgr != 0 && bgr != 1) return fail(c, MDVT_ERR_INVALID_ARG, "bgr must be 0 (RGB) or 1 (BGR), got %d", bgr);
    if (frames_pitch < (size_t)in_w * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "frames_pitch smaller than one row");
    if (n_frames > 1 && frames_stride < frames_pitch * (size_t)in_h) return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    return MDVT_OK;
}

// mdvt_tracker_depth and mdvt_tracker_mask: one body, the divisor's check and the kernel apart
int tracker_plane(mdvt_ctx* c, bool mask, int in_w, int in_h, int n_frames, const uint8_t* d_frames, size_t frames_pitch, size_t frames_stride, int bgr,
                  double max_depth, int mid_w, int mid_h, int out_w, int out_h, float* d_out, size_t out_pitch, size_t out_stride, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (int rc = check_frames_in(c, in_w, in_h, n_frames, d_frames, frames_pitch, frames_stride, bgr, mid_w, mid_h, out_w, out_h, d_out)) return rc;
    if (!mask && !(max_depth > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "max_depth must be > 0");
    if (out_pitch < (size_t)out_w * 4u) return fail(c, MDVT_ERR_INVALID_ARG, "out_pitch smaller than one row");
    if (n_frames > 1 && out_stride < out_pitch * (size_t)out_h) return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if (!multiples_of(4, d_out, out_pitch, n_frames > 1 ? out_stride : (size_t)0))
        return fail(c, MDVT_ERR_INVALID_ARG, "d_out, out_pitch and out_stride must be multiples of 4");
    if ((uint64_t)in_w * (uint64_t)in_h >= ((uint64_t)1 << 31) || (uint64_t)out_w * (uint64_t)out_h >= ((uint64_t)1 << 31))
        return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large (%d x %d -> %d x %d)", in_w, in_h, out_w, out_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) frames_stride = out_stride = 0;
    mdvt::TrackerPlaneArgs a{};
    a.src = d_frames; a.src_pitch = frames_pitch; a.src_stride = frames_stride; a.in_w = in_w; a.in_h = in_h; a.bgr = bgr;
    a.scale_x = size_ratio(in_w, mid_w); a.scale_y = size_ratio(in_h, mid_h);
    a.small = (int64_t)mid_w + (int64_t)mid_h <= 128;               // torch's own choice between its two CPU kernels (include/mdvt_mvsa.h)
    a.divisor = mask ? 255.0f : (float)(4228250625.0 / max_depth);
    a.dst = reinterpret_cast<uint8_t*>(d_out); a.dst_pitch = out_pitch; a.dst_stride = out_stride;
    a.out_w = out_w; a.dst_vec = multiples_of(16, d_out, out_pitch, out_stride);
    a.gw = ((uint32_t)out_w + 3u) / 4u; a.groups = a.gw * (uint32_t)out_h;
    for (int f0 = 0; f0 < n_frames; f0 += kGridFrames) {
        a.frame0 = f0;
        const int n = set_len(n_frames, f0, kGridFrames);
        MDVT_HIP(c, mask ? mdvt::launch_tracker_mask(a, n, s) : mdvt::launch_tracker_depth(a, n, s));
    }
    return MDVT_OK;
}

}  // namespace

extern "C" {

int mdvt_megasam_vector_path(int in_w, int n_frames, const uint8_t* d_frames, size_t frames_pitch, size_t frames_stride)
{
    return in_w >= 6 && multiples_of(16, d_frames, frames_pitch, n_frames > 1 ? frames_stride : (size_t)0) ? 1 : 0;
}

// cv2.resize(INTER_AREA) and a crop into planes.  One scratch block: the two axes' tables.
int mdvt_area_model_frames(mdvt_ctx* c, int in_w, int in_h, int n_frames, const uint8_t* d_frames, size_t frames_pitch, size_t frames_stride, int bgr,
                           int mid_w, int mid_h, int out_w, int out_h, uint8_t* d_out, size_t out_pitch, size_t out_plane_stride, size_t out_stride,
                           void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (int rc = check_frames_in(c, in_w, in_h, n_frames, d_frames, frames_pitch, frames_stride, bgr, mid_w, mid_h, out_w, out_h, d_out)) return rc;
    if (out_pitch < (size_t)out_w) return fail(c, MDVT_ERR_INVALID_ARG, "out_pitch smaller than one row");
    if (out_plane_stride < out_pitch * (size_t)out_h) return fail(c, MDVT_ERR_INVALID_ARG, "out_plane_stride smaller than one plane");
    if (n_frames > 1 && out_stride < out_plane_stride * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if (mid_w > in_w || mid_h > in_h)
        return fail(c, MDVT_ERR_UNSUPPORTED, "area enlargement is another algorithm (%d x %d -> %d x %d)", in_w, in_h, mid_w, mid_h);
    if (whole_ratio(in_w, mid_w) && whole_ratio(in_h, mid_h) && (in_w != mid_w || in_h != mid_h))
        return fail(c, MDVT_ERR_UNSUPPORTED, "integer factors %d x %d: cv2 takes its integer-factor area path, with other rounding, unobserved (%d x %d -> %d x %d)",
                    in_w / mid_w, in_h / mid_h, in_w, in_h, mid_w, mid_h);
    if (in_w > kAreaMaxSize || in_h > kAreaMaxSize) return fail(c, MDVT_ERR_UNSUPPORTED, "size beyond %d (%d x %d)", kAreaMaxSize, in_w, in_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) frames_stride = out_stride = 0;
    mdvt::AreaFramesArgs a{};
    const AreaTable *th = nullptr, *tv = nullptr;
    if (int rc = stage_tables(c, in_w, mid_w, in_h, mid_h, th, tv, a.x, a.y, s)) return rc;
    a.src = d_frames; a.src_pitch = frames_pitch; a.src_stride = frames_stride; a.in_w = in_w; a.bgr = bgr;
    a.src_vec = mdvt_megasam_vector_path(in_w, n_frames, d_frames, frames_pitch, frames_stride);
    a.dst = d_out; a.dst_pitch = out_pitch; a.dst_plane = out_plane_stride; a.dst_stride = out_stride; a.out_w = out_w; a.out_h = out_h;
    // the widest tile, at most a workgroup's 256 columns, whose staged rows fit the LDS
    for (a.tile_w = 256; ; a.tile_w /= 2) {
        a.lds_row = staged_row_bytes(*th, out_w, a.tile_w, a.src_vec != 0);
        if ((size_t)a.lds_row * (size_t)tv->ktaps <= mdvt::kAreaLds) break;
        if (a.tile_w == 1)
            return fail(c, MDVT_ERR_UNSUPPORTED, "the %d source rows of an output row do not fit the LDS even one column wide (%d x %d -> %d x %d)",
                        tv->ktaps, in_w, in_h, mid_w, mid_h);
    }
    for (int f0 = 0; f0 < n_frames; f0 += kGridFrames) {
        a.frame0 = f0;
        MDVT_HIP(c, mdvt::launch_area_frames(a, set_len(n_frames, f0, kGridFrames), s));
    }
    return MDVT_OK;
}

// Depth codes through nearest-exact to the tracker's depth.  No scratch block: launches only.
int mdvt_tracker_depth(mdvt_ctx* c, int in_w, int in_h, int n_frames, const uint8_t* d_frames, size_t frames_pitch, size_t frames_stride, int bgr,
                       double max_depth, int mid_w, int mid_h, int out_w, int out_h, float* d_out, size_t out_pitch, size_t out_stride, void* stream)
{
    return tracker_plane(c, false, in_w, in_h, n_frames, d_frames, frames_pitch, frames_stride, bgr, max_depth, mid_w, mid_h, out_w, out_h, d_out,
                         out_pitch, out_stride, stream);
}

// The inverted grey mask through torch's bilinear resize.  No scratch block: launches only.
int mdvt_tracker_mask(mdvt_ctx* c, int in_w, int in_h, int n_frames, const uint8_t* d_frames, size_t frames_pitch, size_t frames_stride, int bgr,
                      int mid_w, int mid_h, int out_w, int out_h, float* d_out, size_t out_pitch, size_t out_stride, void* stream)
{
    return tracker_plane(c, true, in_w, in_h, n_frames, d_frames, frames_pitch, frames_stride, bgr, 1.0, mid_w, mid_h, out_w, out_h, d_out,
                         out_pitch, out_stride, stream);
}

// The tracker's planes to a depth video's or a grey video's frames.  No scratch block: launches only.
int mdvt_tracker_outputs(mdvt_ctx* c, int mode, int in_w, int in_h, int n_frames, const float* d_planes, size_t planes_pitch, size_t planes_stride,
                         double max_value, int out_w, int out_h, uint8_t* d_frames, size_t frames_pitch, size_t frames_stride, int bgr, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_planes || !d_frames) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (mode != MDVT_TRACKER_DEPTH_VIDEO && mode != MDVT_TRACKER_GREY_VIDEO)
        return fail(c, MDVT_ERR_INVALID_ARG, "mode must be 0 (depth video) or 1 (grey video), got %d", mode);
    if (in_w < 1 || in_h < 1 || out_w < 1 || out_h < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d -> %d x %d", in_w, in_h, out_w, out_h);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (bgr != 0 && bgr != 1) return fail(c, MDVT_ERR_INVALID_ARG, "bgr must be 0 (RGB) or 1 (BGR), got %d", bgr);
    if (!(max_value > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "max_value must be > 0");
    if (planes_pitch < (size_t)in_w * 4u) return fail(c, MDVT_ERR_INVALID_ARG, "planes_pitch smaller than one row");
    if (frames_pitch < (size_t)out_w * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "frames_pitch smaller than one row");
    if (n_frames > 1 && (planes_stride < planes_pitch * (size_t)in_h || frames_stride < frames_pitch * (size_t)out_h))
        return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if (!multiples_of(4, d_planes, planes_pitch, n_frames > 1 ? planes_stride : (size_t)0))
        return fail(c, MDVT_ERR_INVALID_ARG, "d_planes, planes_pitch and planes_stride must be multiples of 4");
    if ((uint64_t)out_w * (uint64_t)out_h >= ((uint64_t)1 << 31))
        return fail(c, MDVT_ERR_UNSUPPORTED, "output frame too large (%d x %d)", out_w, out_h);
    if (mode == MDVT_TRACKER_GREY_VIDEO && in_w == 2 * (int64_t)out_w && in_h == 2 * (int64_t)out_h)
        return fail(c, MDVT_ERR_UNSUPPORTED, "an exact 2 x reduction: cv2 takes its area mean there (%d x %d -> %d x %d)", in_w, in_h, out_w, out_h);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) planes_stride = frames_stride = 0;
    mdvt::TrackerOutArgs a{};
    a.c.src = reinterpret_cast<const uint8_t*>(d_planes); a.c.src_pitch = planes_pitch; a.c.src_stride = planes_stride; a.c.in_w = in_w; a.c.in_h = in_h;
    a.c.src_vec = multiples_of(16, d_planes, planes_pitch, planes_stride);
    a.c.fmax = (float)max_value; a.c.multi = 4228250625.0 / max_value;
    a.c.out_w = out_w; a.c.out_h = out_h; a.c.resize = in_w != out_w || in_h != out_h;
    a.c.ratio_x = (double)in_w / (double)out_w; a.c.ratio_y = (double)in_h / (double)out_h;
    a.c.codes = d_frames; a.c.codes_pitch = frames_pitch; a.c.codes_stride = frames_stride; a.c.bgr = bgr;
    a.c.codes_vec = multiples_of(4, d_frames, frames_pitch, frames_stride);
    a.c.gw = ((uint32_t)out_w + 3u) / 4u; a.c.groups = a.c.gw * (uint32_t)out_h;
    a.scale_x = size_ratio(in_w, out_w); a.scale_y = size_ratio(in_h, out_h);
    for (int f0 = 0; f0 < n_frames; f0 += kGridFrames) {
        a.c.frame0 = f0;
        const int n = set_len(n_frames, f0, kGridFrames);
        MDVT_HIP(c, mode == MDVT_TRACKER_GREY_VIDEO ? mdvt::launch_tracker_grey(a, n, s) : mdvt::launch_tracker_codes(a, n, s));
    }
    return MDVT_OK;
}

}  // extern "C"
