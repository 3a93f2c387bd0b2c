// mdvt_ffv1_host.h -- what the parts of the host codec (libmdvt_video.so) share: the error channel of the C ABI, the exception
// barrier, the slice thread pool, the FFV1 parameters, and the interfaces of the decoder (mdvt_ffv1_dec.cpp) and the encoders
// (mdvt_ffv1_enc.cpp).  The FFV1 primitives themselves -- CRC, state tables, range decoder, bit reader, Golomb-Rice symbols,
// predictor, pixel stores -- are csrc/mdvt_ffv1_core.h's, shared with the device.  Internal: nothing here is part of the ABI.
#pragma once

#include "mdvt_ffv1_core.h"

#pragma GCC visibility push(default)          // the library is built with hidden visibility: the ABI alone is exported
#include "mdvt_video.h"
#include "mdvt_video_stream.h"
#pragma GCC visibility pop

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <exception>
#include <new>
#include <string>
#include <thread>
#include <vector>

namespace mdvt_host {

using namespace mdvt_ffv1;

// ---------------------------------------------------------------------------------------------------------------------
// errors: a negative code and the calling thread's message (mdvt_video_last_error)
// ---------------------------------------------------------------------------------------------------------------------
enum { ERR_ARG = -1, ERR_IO = -2, ERR_FORMAT = -3, ERR_UNSUPPORTED = -4, ERR_DATA = -5 };

inline thread_local std::string g_err;

inline int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// The exception barrier: every extern "C" body and every slice thread runs inside it, so that no exception crosses the C ABI or
// ends a thread.  (The out-of-memory message fits the string's own buffer: reporting it allocates nothing.)
template <class Body>
int guarded(Body&& body) noexcept
{
    try {
        try { return body(); }
        catch (const std::bad_alloc&) { throw; }
        catch (const std::exception& e) { return fail(ERR_DATA, "unexpected exception: %s", e.what()); }
        catch (...) { return fail(ERR_DATA, "unexpected exception"); }
    } catch (...) { return fail(ERR_IO, "out of memory"); }
}

// n slice jobs on up to `threads` std::threads (0: one per core, never more than n); job(i) -> 0 or a code from fail().
// -> 0, or a failing job's code with its thread's message brought back to the caller's
template <class Job>
int run_slices(int n, int threads, Job job)
{
    std::atomic<int> next(0), failed(0);
    auto work = [&]() {
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= n) return 0;
            const int rc = job(i);
            if (rc) failed = rc;
        }
    };
    int nt = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    nt = std::max(1, std::min(nt, n));
    if (nt == 1) { work(); return failed; }
    std::vector<std::thread> th;
    std::vector<std::string> errs((size_t)nt);
    for (int t = 0; t < nt; ++t)
        th.emplace_back([&, t]() {
            const int rc = guarded([&]() { work(); errs[(size_t)t] = g_err; return 0; });
            if (rc) failed = rc;
        });
    for (auto& t : th) t.join();
    if (failed) for (auto& e : errs) if (!e.empty()) g_err = e;
    return failed;
}

// ---------------------------------------------------------------------------------------------------------------------
// FFV1 parameters
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kMaxQuantTables = 8, kContextSize = 32, kMaxContextInputs = 5;

struct Ffv1Config {
    int version = -1, micro = 0, coder = 0, colorspace = 0, bits = 8, chroma_planes = 1, hshift = 0, vshift = 0, alpha = 0;
    int nh = 1, nv = 1, qcount = 1, ec = 0, intra = 0;
    int16_t quant[kMaxQuantTables][kMaxContextInputs][256];
    int context_count[kMaxQuantTables] = {0};
    std::vector<uint8_t> initial_states[kMaxQuantTables];      // context_count * 32, empty = all 128
    uint16_t next[256];                                        // the state table of the slices' range coders (RacDec::next)
    int plane_count() const { return 2 + alpha; }              // Y, the two chroma planes share one context set, alpha
    bool ycbcr() const { return colorspace == 0; }
    int pix_fmt() const { return !ycbcr() ? MDVT_VIDEO_PIX_RGB : vshift ? MDVT_VIDEO_PIX_YUV420P : hshift ? MDVT_VIDEO_PIX_YUV422P : MDVT_VIDEO_PIX_YUV444P; }
};

inline VlcState fresh_vlc() { VlcState v; vlc_reset(&v); return v; }

// the context of a sample from its neighbours: q = one set of five tables, `five` when the last two are in use
struct LineCtx {
    const int16_t (*q)[256];
    bool five;
};

inline int get_context(const LineCtx& lc, const int16_t* src, const int16_t* last, const int16_t* last2)
{
    const int LT = last[-1], T = last[0], RT = last[1], L = src[-1];
    int ctx = lc.q[0][(L - LT) & 0xFF] + lc.q[1][(LT - T) & 0xFF] + lc.q[2][(T - RT) & 0xFF];
    if (lc.five) ctx += lc.q[3][(src[-2] - L) & 0xFF] + lc.q[4][(last2[0] - T) & 0xFF];
    return ctx;
}

// ---------------------------------------------------------------------------------------------------------------------
// decoder (mdvt_ffv1_dec.cpp)
// ---------------------------------------------------------------------------------------------------------------------
// per-slice context state, kept between the frames of a non-intra stream
struct PlaneState { int qidx = 0; std::vector<uint8_t> state; std::vector<VlcState> vlc; };
struct SliceState { PlaneState plane[3]; };

// the configuration record (RFC 9043 section 4.2); for versions 0 / 1 the same fields sit inside the key frame
int parse_config_record(const uint8_t* data, size_t size, Ffv1Config& f);

struct Decoder {
    Ffv1Config f;
    int W = 0, H = 0;
    bool have_config = false;          // version >= 2: from the container; versions 0 / 1: from the first key frame
    bool key_frame_ok = false;
    std::vector<SliceState> slices;

    int check_supported() const;
    int decode_frame(const uint8_t* pkt, size_t size, uint8_t* dst, size_t pitch, int order, int threads);
};

// ---------------------------------------------------------------------------------------------------------------------
// encoders (mdvt_ffv1_enc.cpp): version 3.4, RGB, 8 bits, ec = 1, the default 666-context tables
// ---------------------------------------------------------------------------------------------------------------------
// (colorspace 0 with its chroma shifts: tools/ffv1_ycbcr_writer.cpp, which makes YCbCr streams for measurements; no writer of this library's does)
std::vector<uint8_t> make_config_record(int nh, int nv, int coder = 1, int intra = 1, int colorspace = 1, int hshift = 0, int vshift = 0);

// the range coder with the default state table, every frame a key frame
int encode_frame(int W, int H, int nh, int nv, const uint8_t* src, size_t pitch, int order, int threads, std::vector<uint8_t>& packet);

// Golomb-Rice with run mode, intra = 0: a slice's VlcStates (luma, chroma) carry from frame to frame and are reset at a key frame
struct GolombSliceState { std::vector<VlcState> vlc[2]; };
int encode_frame_golomb(int W, int H, int nh, int nv, const uint8_t* src, size_t pitch, int order, int threads, bool key,
                        std::vector<GolombSliceState>& states, std::vector<uint8_t>& packet);

// The parts of a Golomb-Rice slice, for encode_frame_golomb and the YCbCr measurement tool:
struct BitWriter {
    std::vector<uint8_t> out;
    uint64_t acc = 0;
    int n = 0;
    inline void put(int bits, uint32_t v)        // bits <= 32
    {
        acc = (acc << bits) | v; n += bits;
        while (n >= 8) { out.push_back((uint8_t)(acc >> (n - 8))); n -= 8; }
    }
    void flush() { if (n) { out.push_back((uint8_t)(acc << (8 - n))); n = 0; } }
};
// the slice's range-coded start: the key-frame bit (first slice only), the slice header, the sentinel bit behind which the bit stream begins
std::vector<uint8_t> golomb_slice_start(int sx, int sy, bool first, bool key);
// fresh VlcStates where a key-frame run begins (or nothing is there yet)
void begin_golomb_run(GolombSliceState& ss, bool key);
// one line of w samples of kBits (8 or 9) bits: cur[-1], last[-1 .. w] are set; run_index runs on from line to line
template <int kBits>
void encode_line_golomb(BitWriter& bw, VlcState* vlc, const int16_t* cur, const int16_t* last, int w, int& run_index);
// closes a slice: its 24-bit payload size, the error-status byte, the CRC-32 parity
void close_slice(std::vector<uint8_t>& out);

}  // namespace mdvt_host
