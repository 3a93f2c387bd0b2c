// mdvt_infill_engines.hip -- the input stage of the m2svid infill step (include/mdvt_infill_engines.h): the reference's per-frame
// host code of m2svid_infill.py:224-261 ("m2s").  The step's other half, mdvt_model_infill_finish, runs on the listed-pixel stages
// of mdvt_normal_infill.hip.
//
//   k_m2s_prepare   m2s:224-261   an eye of the side-by-side colour and mask frames and the original frame -> the model's image, its
//                                 original image (both image_w x image_h) and its mask (mask_w x mask_h), the left eye's read
//                                 mirrored, and the holes of each model mask
// One launch covers the three outputs: the grid's third dimension is 3 * frame + role (0 image, 1 original image, 2 mask), a thread
// works out one output pixel and fetches only the source pixels that pixel needs (four for the linear resize, whatever the
// ratio: cv2's INTER_LINEAR does not average the pixels in between).  The u8 resize is mdvt_adapter_resize.h's.
//
// The unit is compiled with -ffp-contract=off and without fast-math (Makefile): every `*`, `+` and `-` below is one IEEE operation.
#include "mdvt_device.h"
#include "mdvt_adapter_resize.h"

namespace mdvt {
namespace {

__global__ void __launch_bounds__(256) k_m2s_prepare(M2sPrepareArgs a)
{
    const int role = (int)(blockIdx.z % 3u);                     // (workgroup-uniform)
    const size_t f = blockIdx.z / 3u;
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const int mirror = a.mirror;
    if (role < 2) {                                              // m2s:234-241, 254-261
        const AdapterResize& rs = role == 0 ? a.rs_image : a.rs_org;
        if (x >= rs.out_w || y >= rs.out_h) return;
        const AdapterImage& in = role == 0 ? a.color : a.org;
        const uint8_t* src = in.p + f * in.stride;
        const size_t pitch = in.pitch;
        const int last = rs.in_w - 1;
        const uint32_t c = adapter_resize_px(rs, x, y, [&](int sx, int sy) {
            return load_px_bytes(src + (size_t)sy * pitch, mirror ? last - sx : sx);
        });
        uint8_t* out = role == 0 ? a.image + f * a.image_stride + (size_t)y * a.image_pitch
                                 : a.org_image + f * a.org_image_stride + (size_t)y * a.org_image_pitch;
        store_px_bytes(out, x, c);
        return;
    }
    bool hole = false;                                           // m2s:226-231, 244-251
    if (x < a.rs_mask.out_w && y < a.rs_mask.out_h) {
        const uint8_t* mask = a.mask.p + f * a.mask.stride;
        const size_t pitch = a.mask.pitch;
        const int last = a.rs_mask.in_w - 1;
        const uint32_t m = adapter_resize_px(a.rs_mask, x, y, [&](int sx, int sy) {
            return load_px_bytes(mask + (size_t)sy * pitch, mirror ? last - sx : sx) != 0u ? 255u : 0u;      // m2s:227, 245
        });
        hole = m != 0u;                                                                                        // m2s:229, 249: > 0
        a.mmask[f * a.mmask_stride + (size_t)y * a.mmask_pitch + x] = hole ? 255 : 0;
    }
    const unsigned long long b = __ballot(hole);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(a.holes + f, (uint32_t)__popcll(b));
}

}  // namespace

hipError_t launch_m2s_prepare(const M2sPrepareArgs& a, int n, hipStream_t s)
{
    const int w = a.rs_image.out_w > a.rs_mask.out_w ? a.rs_image.out_w : a.rs_mask.out_w;
    const int h = a.rs_image.out_h > a.rs_mask.out_h ? a.rs_image.out_h : a.rs_mask.out_h;
    hipLaunchKernelGGL(k_m2s_prepare, dim3((w + 255) / 256, h, 3 * n), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdvt
