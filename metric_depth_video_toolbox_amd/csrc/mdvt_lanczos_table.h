// mdvt_lanczos_table.h -- the coefficient and bounds table of one axis of Pillow's 8-bit Lanczos resampler (Resample.c: precompute_coeffs,
// normalize_coeffs_8bpc), built on the host in double with the C library's sin, as Pillow builds it: a device sin is not promised to
// give its bits.  Plain C++ with no HIP in it, so that a stand-alone host program can hold it to the restatement of
// tests/video_mask_ref.py (tests/lanczos_table_host.cpp).  include/mdvt_video_mask.h states the arithmetic.
#pragma once

#include <math.h>
#include <stdint.h>

#include <vector>

namespace mdvt::host {

constexpr int kLanczosPrecisionBits = 22;       // 32 - 8 - 2 (Resample.c: PRECISION_BITS)
constexpr int kLanczosMaxSize = 8192;           // the largest `in` and `out` a table is built for

struct LanczosTable {
    int in = 0, out = 0, ksize = 0;
    std::vector<int32_t> bounds;                // [out][2]: the first source sample, the number of taps
    std::vector<int32_t> coef;                  // [ksize][out]: tap x of output xx at x * out + xx (neighbouring outputs, neighbouring words)
};

inline double lanczos_filter(double x)
{
    auto sinc = [](double t) { return t == 0.0 ? 1.0 : sin(t * M_PI) / (t * M_PI); };
    return -3.0 <= x && x < 3.0 ? sinc(x) * sinc(x / 3.0) : 0.0;
}

// Fills `t` for `in` samples resized to `out`.  false: a size out of range, or an output whose 255 * sum|k| + 2^21 would not fit an
// int32 (for this filter none does; the kernels' sums rest on it, so it is checked where the table is made).
inline bool build_lanczos_table(int in, int out, LanczosTable& t)
{
    if (in < 1 || out < 1 || in > kLanczosMaxSize || out > kLanczosMaxSize) return false;
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 3.0 * fs;
    const int ksize = 2 * (int)ceil(support) + 1;
    t.in = in; t.out = out; t.ksize = ksize;
    t.bounds.assign((size_t)out * 2, 0);
    t.coef.assign((size_t)ksize * (size_t)out, 0);
    std::vector<double> w((size_t)ksize);
    const double ss = 1.0 / fs;
    for (int xx = 0; xx < out; ++xx) {
        const double center = ((double)xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        if (xmax < 0) xmax = 0;
        if (xmax > ksize) return false;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[(size_t)x] = lanczos_filter(((double)(x + xmin) - center + 0.5) * ss);
            ww += w[(size_t)x];
        }
        int64_t mag = 0;
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) w[(size_t)x] /= ww;
            const double v = w[(size_t)x];
            const int32_t k = (int32_t)(v * (double)(1 << kLanczosPrecisionBits) + (v < 0.0 ? -0.5 : 0.5));     // truncation toward zero
            t.coef[(size_t)x * (size_t)out + (size_t)xx] = k;
            mag += k < 0 ? -(int64_t)k : (int64_t)k;
        }
        if (255 * mag + ((int64_t)1 << (kLanczosPrecisionBits - 1)) >= ((int64_t)1 << 31)) return false;
        t.bounds[2 * (size_t)xx] = xmin;
        t.bounds[2 * (size_t)xx + 1] = xmax;
    }
    return true;
}

}  // namespace mdvt::host
