// mdvt_api_scene.hip -- the entry points of include/mdvt_scene.h: the hue, saturation and value difference sums of consecutive
// frames (kernels: mdvt_scene.hip).  The refusals stand in the order the caller meets their texts, each fail(...) text at its
// check; the layout tests are mdvt_context.h's.  Host code only.
#include "mdvt_context.h"
#include "mdvt_scene.h"

using namespace mdvt;
using namespace mdvt::host;

namespace {

// n / factor rounded to the nearest integer, a tie to the even one (Python's round of the quotient)
inline int analysed_size(int n, int factor)
{
    const int q = n / factor, r = n % factor;
    return 2 * (int64_t)r > factor ? q + 1 : (2 * (int64_t)r == factor ? q + (q & 1) : q);
}

}  // namespace

extern "C" {

int mdvt_scene_vector_path(int n_frames, const uint8_t* d_frames, size_t pitch, size_t stride, const uint8_t* d_prev, size_t prev_pitch, int factor)
{
    return factor == 1 && multiples_of(16, d_frames, pitch, n_frames > 1 ? stride : (size_t)0) &&
           (!d_prev || multiples_of(16, d_prev, prev_pitch)) ? 1 : 0;
}

// No scratch block: one memset and one launch.
int mdvt_scene_frame_sums(mdvt_ctx* c, int width, int height, int n_frames, const uint8_t* d_frames, size_t pitch, size_t stride, int order,
                          const uint8_t* d_prev, size_t prev_pitch, int factor, uint64_t* d_sums, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_frames || !d_sums) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (!multiples_of(8, d_sums)) return fail(c, MDVT_ERR_INVALID_ARG, "d_sums must be 8-byte aligned");
    if (width < 1 || height < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad size %d x %d", width, height);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (n_frames == 1 && !d_prev) return fail(c, MDVT_ERR_INVALID_ARG, "one frame and no previous frame: no pair to compare");
    if (order != 0 && order != 1) return fail(c, MDVT_ERR_INVALID_ARG, "order must be 0 (RGB) or 1 (BGR), got %d", order);
    if (pitch < (size_t)width * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (d_prev && prev_pitch < (size_t)width * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "prev_pitch smaller than one row");
    if (n_frames > 1 && stride < pitch * (size_t)height) return fail(c, MDVT_ERR_INVALID_ARG, "stride smaller than one frame");
    if (factor < 1) return fail(c, MDVT_ERR_INVALID_ARG, "factor must be >= 1, got %d", factor);
    const int aw = analysed_size(width, factor), ah = analysed_size(height, factor);
    if (aw < 1 || ah < 1) return fail(c, MDVT_ERR_INVALID_ARG, "factor %d leaves a %d x %d image of a %d x %d frame", factor, aw, ah, width, height);
    if ((uint64_t)width * (uint64_t)height > ((uint64_t)1 << 28)) return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large (%d x %d)", width, height);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) stride = 0;
    const int pairs = n_frames - 1 + (d_prev ? 1 : 0);
    const bool vec = mdvt_scene_vector_path(n_frames, d_frames, pitch, stride, d_prev, prev_pitch, factor) != 0;
    mdvt::SceneArgs a{};
    a.frames = d_frames; a.pitch = pitch; a.stride = stride; a.prev = d_prev; a.prev_pitch = d_prev ? prev_pitch : 0;
    a.n_frames = n_frames; a.bgr = order; a.W = (uint32_t)width;
    a.rs = mdvt::adapter_resize(width, height, aw, ah);
    a.gw = ((uint32_t)width + 15u) / 16u;
    a.units = vec ? a.gw * (uint32_t)height : (uint32_t)aw * (uint32_t)ah;
    a.sums = reinterpret_cast<unsigned long long*>(d_sums);
    MDVT_HIP(c, hipMemsetAsync(d_sums, 0, (size_t)pairs * 3u * sizeof(uint64_t), s));
    MDVT_HIP(c, mdvt::launch_scene_sums(a, vec, s));
    return MDVT_OK;
}

}  // extern "C"
