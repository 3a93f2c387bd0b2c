// mdvt_depth_sink.hip -- metric depth planes to the 16-bit RGB codes of a depth video (mdvt_depth_video_codes;
// include/mdvt_depth_sink.h): depth_frames_helper.save_depth_video (dfh:125-161) behind an optional NaN rule (moge_video.py:171) and an
// optional factor that lives on the device (video_da3.py:193), bit for bit.  The sink of every metric-depth script of the reference.
//
// The unit is compiled with -ffp-contract=off and without fast-math (Makefile): every `*` and `+` below is one IEEE operation,
// rounded before the next.  Shared with mdvt_metric_align.hip's k_metric_codes through mdvt_depth_code.h: the frame (quad_of), the
// float32 gather with its resize tables (quad_values) and the tail (codes_out: clip, code, packed stores).  This unit's own: prepare,
// the function of a source value, and the LDS-staged upscale.
//
// k_depth_sink: a thread per four output pixels of a row, a frame per blockIdx.y.
// Same size: one 16-byte load of four source values where the plane's address, pitch and stride are multiples of 16, element by element
// otherwise.  Resized: each output pixel prepares its up to four source values, filters horizontally then vertically; where the
// source is no wider than the output (the usual direction) k_depth_sink_up stages the two source rows of a workgroup in LDS first.
// Then clip and code: 12 bytes of codes as three dword stores and four plane values as one 16-byte store where the output's address,
// pitch and stride allow, byte by byte and value by value otherwise.  A value's arithmetic does not depend on which kernel, loads and
// stores it takes, nor on the launch geometry.
#include "mdvt_internal.h"
#include "mdvt_depth_code.h"

namespace mdvt {
namespace {

using depth_code::tap;
using depth_code::Quad;
using depth_code::quad_of;
using depth_code::quad_values;
using depth_code::codes_out;

// steps 1 and 2 of the header on a source value
__device__ __forceinline__ float prepare(float x, bool nan_to_max, bool scaled, float s, float fmax)
{
    if (nan_to_max && x != x) x = fmax;
    return scaled ? x * s : x;
}

template <bool RESIZE>
__global__ void __launch_bounds__(256) k_depth_sink(DepthCodesArgs a)
{
    Quad q;
    if (!quad_of(a.groups, a.gw, a.out_w, a.frame0, q)) return;
    const bool ntm = a.nan_to_max != 0, scaled = a.scale != nullptr;
    const float s = scaled ? *a.scale : 1.0f, fmax = a.fmax;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    quad_values(d, a.src + q.f * a.src_stride, a.src_pitch, a.src_vec != 0, q, RESIZE, a.ratio_x, a.ratio_y, a.in_w, a.in_h,
                [=](float x) { return prepare(x, ntm, scaled, s, fmax); });
    codes_out(d, q, a);
}

// The resize where a source row is no longer than an output row (in_w <= out_w: the models' sizes to a video's).  A workgroup takes up
// to 256 groups of ONE output row: its lanes' taps lie in one span of the two source rows, at most kUpSpan values each (below), which
// the workgroup brings into LDS with coalesced loads, each value prepared once; the lanes then filter from LDS.  Measured
// (profiles/r17_depth_sink.md): k_depth_sink<true>'s gathers cost by the cache lines a wave's load touches -- 4.7 ps per output pixel
// with no reuse, 2.4 at 2 x, 1.95 at 4 x -- and the rows in LDS take 128 planes of 924x518 -> 1920x1080 from 0.64 to 0.55 ms and
// change nothing at 4 x: what is left, about 2 ps per pixel, does not depend on the loads.  The arithmetic per value is
// k_depth_sink<true>'s, operation for operation.
//
// The span: a workgroup's output columns are at most 1023 apart and in / out <= 1, so the exact tap positions are at most 1023 apart;
// fx is rounded to float32, which below 2^22 (launch_depth_sink sends wider sources to k_depth_sink<true>) moves it by at most 0.25:
// floor differs by at most 1024, the second tap adds 1, so a span holds at most 1026 values.
constexpr int kUpSpan = 1032;

__global__ void __launch_bounds__(256) k_depth_sink_up(DepthCodesArgs a)
{
    __shared__ float s_r0[kUpSpan], s_r1[kUpSpan];
    const uint32_t cpr = (a.gw + 255u) / 256u;                      // workgroups per output row
    const uint32_t row = blockIdx.x / cpr, g0 = (blockIdx.x - row * cpr) * 256u;
    const uint32_t ng = a.gw - g0 < 256u ? a.gw - g0 : 256u;        // groups of this workgroup: 1 .. 256
    const size_t f = (size_t)a.frame0 + blockIdx.y;
    const bool ntm = a.nan_to_max != 0, scaled = a.scale != nullptr;
    const float s = scaled ? *a.scale : 1.0f;
    const uint8_t* src = a.src + f * a.src_stride;
    int y0, y1;
    float b0, b1;
    tap((int)row, a.ratio_y, a.in_h, y0, y1, b0, b1);
    const float* r0 = reinterpret_cast<const float*>(src + (size_t)y0 * a.src_pitch);
    const float* r1 = reinterpret_cast<const float*>(src + (size_t)y1 * a.src_pitch);
    const int x_first = (int)(4u * g0);
    const uint32_t x_end = 4u * (g0 + ng);                         // <= out_w + 3: unsigned, an int would wrap for out_w above 2^31 - 4
    const int x_last = (int)((x_end < (uint32_t)a.out_w ? x_end : (uint32_t)a.out_w) - 1u);
    int base, last, unused_i;
    float unused_f0, unused_f1;
    tap(x_first, a.ratio_x, a.in_w, base, unused_i, unused_f0, unused_f1);
    tap(x_last, a.ratio_x, a.in_w, unused_i, last, unused_f0, unused_f1);
    const int span = last - base + 1;                               // 1 .. 1026 (above); base + span <= in_w
    for (int i = (int)threadIdx.x; i < span; i += 256) {
        s_r0[i] = prepare(r0[base + i], ntm, scaled, s, a.fmax);
        s_r1[i] = prepare(r1[base + i], ntm, scaled, s, a.fmax);
    }
    __syncthreads();
    if (threadIdx.x >= ng) return;
    const int x0 = x_first + 4 * (int)threadIdx.x;
    const Quad q{row, x0, a.out_w - x0 < 4 ? a.out_w - x0 : 4, f};
    float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < q.nv) {
            int s0, s1;
            float a0, a1;
            tap(x0 + k, a.ratio_x, a.in_w, s0, s1, a0, a1);
            s0 -= base; s1 -= base;
            const float h0 = s_r0[s0] * a0 + s_r0[s1] * a1;
            const float h1 = s_r1[s0] * a0 + s_r1[s1] * a1;
            d[k] = h0 * b0 + h1 * b1;
        }
    }
    codes_out(d, q, a);
}

}  // namespace

hipError_t launch_depth_sink(const DepthCodesArgs& a, int n_frames, hipStream_t s)
{
    if (a.resize && a.in_w <= a.out_w && a.in_w < (1 << 22)) {
        const dim3 grid(((a.gw + 255u) / 256u) * (unsigned)a.out_h, (unsigned)n_frames);
        hipLaunchKernelGGL(k_depth_sink_up, grid, dim3(256), 0, s, a);
        return hipGetLastError();
    }
    const dim3 grid((a.groups + 255u) / 256u, (unsigned)n_frames);
    if (a.resize) hipLaunchKernelGGL(k_depth_sink<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_depth_sink<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdvt
