// mdvt_area_table.h -- the tap table of one axis of cv2.resize(INTER_AREA)'s general (non-integer) path (OpenCV's computeResizeAreaTab,
// restated, not observed), built on the host in double with each weight rounded to float32 once, as OpenCV stores it.  Plain C++ with
// no HIP in it, so that a stand-alone host program can hold it to the restatement of tests/megasam_ref.py
// (tests/area_table_host.cpp).  include/mdvt_megasam.h states the arithmetic.
#pragma once

#include <math.h>
#include <stdint.h>

#include <vector>

namespace mdvt::host {

constexpr int kAreaMaxSize = 16384;             // the largest `in` and `out` a table is built for

struct AreaTable {
    int in = 0, out = 0, ktaps = 0;             // ktaps: the most taps any output takes
    std::vector<int32_t> first;                 // [out]: the first source sample of output d
    std::vector<int32_t> count;                 // [out]: its taps, 1 .. ktaps, on consecutive source samples
    std::vector<float> w;                       // [out][ktaps]: tap k of output d at d * ktaps + k, 0 behind count[d]
};

// Fills `t` for `in` samples reduced to `out`.  false: a size out of range or an enlargement (out > in).
inline bool build_area_table(int in, int out, AreaTable& t)
{
    if (in < 1 || out < 1 || in > kAreaMaxSize || out > in) return false;
    const double scale = (double)in / (double)out;
    t.in = in; t.out = out;
    t.first.assign((size_t)out, 0);
    t.count.assign((size_t)out, 0);
    std::vector<std::vector<float>> taps((size_t)out);
    int ktaps = 1;
    for (int d = 0; d < out; ++d) {
        const double f1 = (double)d * scale, f2 = f1 + scale;
        const double rest = (double)in - f1;
        const double cell = scale < rest ? scale : rest;
        int s1 = (int)ceil(f1), s2 = (int)floor(f2);
        if (s2 > in - 1) s2 = in - 1;
        if (s1 > s2) s1 = s2;
        std::vector<float>& a = taps[(size_t)d];
        int first = s1;
        if ((double)s1 - f1 > 1e-3) {
            first = s1 - 1;
            a.push_back((float)(((double)s1 - f1) / cell));
        }
        for (int s = s1; s < s2; ++s) a.push_back((float)(1.0 / cell));
        if (f2 - (double)s2 > 1e-3) {
            double e = f2 - (double)s2;
            if (e > 1.0) e = 1.0;
            if (e > cell) e = cell;
            a.push_back((float)(e / cell));
        }
        // (no size in range gives any of these; the kernels read first .. first + count - 1 on the table's word)
        if (a.empty() || first < 0 || first + (int)a.size() > in) return false;
        t.first[(size_t)d] = first;
        t.count[(size_t)d] = (int32_t)a.size();
        if ((int)a.size() > ktaps) ktaps = (int)a.size();
    }
    t.ktaps = ktaps;
    t.w.assign((size_t)out * (size_t)ktaps, 0.0f);
    for (int d = 0; d < out; ++d)
        for (size_t k = 0; k < taps[(size_t)d].size(); ++k) t.w[(size_t)d * (size_t)ktaps + k] = taps[(size_t)d][k];
    return true;
}

}  // namespace mdvt::host
