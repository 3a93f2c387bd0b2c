// mdvt_video.cpp -- FFV1 (RFC 9043) in Matroska (RFC 9559 / EBML RFC 8794), reader and writer: the C ABI of include/mdvt_video.h.
//
// Host C++17, no third-party library.  What the reference does with OpenCV's FFmpeg back end -- cv2.VideoCapture over the
// toolbox's *_depth.mkv files (stereo_rerender.py:326-341) and cv2.VideoWriter(fourcc 'FFV1') for the stereo / infill-mask /
// depth outputs (stereo_rerender.py:426-444, 941; depth_frames_helper.py:125-161) -- written from the specifications:
//
//   decoder   FFV1 versions 0, 1 (global header inside every key frame, one slice) and 3 (configuration record in the
//             container's CodecPrivate, N slices per frame, each followed by its 24-bit size, an error-status byte and a CRC-32
//             parity when ec = 1); coder_type 0 (Golomb-Rice with run mode), 1 (range coder, default state-transition table) and
//             2 (custom table sent as deltas); colorspace_type 1 (JPEG 2000 RCT over 8-bit R, G, B, +- alpha: what FFmpeg codes
//             for bgr0 / bgra, the pixel format OpenCV feeds FFV1) and colorspace_type 0 (YCbCr, 8 bits, chroma subsampled by
//             (0, 0), (1, 0) or (1, 1): yuv444p, yuv422p, yuv420p -- FFmpeg's default for a movie -- converted to RGB as
//             include/mdvt_video.h states it); key frames AND inter frames (inter frames keep the context states of the previous
//             frame, so the stream is read in order).  Grey, alpha beside YCbCr and more than 8 bits are refused with a message.
//   encoder   version 3.4, coder_type 1, intra-only, RGB colour space, 8 bits, slices_h x slices_v slices, ec = 1; the
//             quantisation tables FFmpeg's encoder uses for 8-bit input (quant11, context model 0: 666 contexts).
//   container one video track, CodecID V_FFV1 with the configuration record as CodecPrivate (reader also: V_MS/VFW/FOURCC with a
//             BITMAPINFOHEADER 'FFV1' followed by the record, or nothing for versions 0 / 1), SimpleBlocks (reader also: BlockGroups)
//             in Clusters, Cues at the end, Duration and Segment size patched on finish.
//
// Slices are decoded / encoded on std::threads (one per slice up to the host's cores).
#include "mdvt_video.h"
#include "mdvt_video_stream.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <string>
#include <thread>
#include <vector>

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

enum { ERR_ARG = -1, ERR_IO = -2, ERR_FORMAT = -3, ERR_UNSUPPORTED = -4, ERR_DATA = -5 };

// ---------------------------------------------------------------------------------------------------------------------
// CRC-32, generator 0x04C11DB7, most significant bit first, initial value 0, no final XOR (RFC 9043 section 4.9.3 / 4.3)
// ---------------------------------------------------------------------------------------------------------------------
struct CrcTable {
    uint32_t t[256];
    CrcTable()
    {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i << 24;
            for (int k = 0; k < 8; ++k) c = (c << 1) ^ ((c & 0x80000000u) ? 0x04C11DB7u : 0u);
            t[i] = c;
        }
    }
};
const CrcTable g_crc;

uint32_t crc32_msb(uint32_t crc, const uint8_t* p, size_t n)
{
    for (size_t i = 0; i < n; ++i) crc = (crc << 8) ^ g_crc.t[(crc >> 24) ^ p[i]];
    return crc;
}

// ---------------------------------------------------------------------------------------------------------------------
// Range coder (RFC 9043 section 3.8.1): binary, adaptive 8-bit states, byte-wise renormalisation
// ---------------------------------------------------------------------------------------------------------------------
struct StateTables { uint8_t zero[256], one[256]; };

// default_state_transition (RFC 9043 section 3.8.1.3), generated the way FFmpeg's ff_build_rac_states(0.05 * 2^32, 256 - 8)
// generates it; tests/test_ffv1_cpu.py checks it against the RFC's table (its first and last rows are quoted there).
void build_default_states(StateTables& s)
{
    const int64_t one = 1LL << 32;
    const int factor = (int)(0.05 * (double)(1LL << 32));
    const int max_p = 256 - 8;
    memset(s.zero, 0, sizeof s.zero);
    memset(s.one, 0, sizeof s.one);
    int last_p8 = 0;
    int64_t p = one / 2;
    for (int i = 0; i < 128; ++i) {
        int p8 = (int)((256 * p + one / 2) >> 32);
        if (p8 <= last_p8) p8 = last_p8 + 1;
        if (last_p8 && last_p8 < 256 && p8 <= max_p) s.one[last_p8] = (uint8_t)p8;
        p += ((one - p) * factor + one / 2) >> 32;
        last_p8 = p8;
    }
    for (int i = 256 - max_p; i <= max_p; ++i) {
        if (s.one[i]) continue;
        p = (i * one + 128) >> 8;
        p += ((one - p) * factor + one / 2) >> 32;
        int p8 = (int)((256 * p + one / 2) >> 32);
        if (p8 <= i) p8 = i + 1;
        if (p8 > max_p) p8 = max_p;
        s.one[i] = (uint8_t)p8;
    }
    for (int i = 1; i < 255; ++i) s.zero[i] = (uint8_t)(256 - s.one[256 - i]);
}

void tables_from_one_state(StateTables& s, const uint8_t* one)      // custom table (coder_type 2)
{
    memcpy(s.one, one, 256);
    s.zero[0] = 0;
    for (int i = 1; i < 256; ++i) s.zero[i] = (uint8_t)(256 - s.one[256 - i]);
}

struct StateTablesDefault : StateTables { StateTablesDefault() { build_default_states(*this); } };
const StateTablesDefault g_default_states;

struct RacDec {
    const uint8_t* start = nullptr; const uint8_t* p = nullptr; const uint8_t* end = nullptr;
    int low = 0, range = 0;
    int overread = 0;
    const StateTables* tab = &g_default_states;
    bool init(const uint8_t* buf, size_t size)
    {
        if (size < 2) return false;
        start = buf; p = buf + 2; end = buf + size;
        low = (buf[0] << 8) | buf[1];
        range = 0xFF00;
        overread = 0;
        if (low >= 0xFF00) { low = 0xFF00; end = p; }
        return true;
    }
    inline int get(uint8_t* state)
    {
        const int range1 = (range * (*state)) >> 8;
        range -= range1;
        int bit;
        if (low < range) { *state = tab->zero[*state]; bit = 0; }
        else { low -= range; range = range1; *state = tab->one[*state]; bit = 1; }
        if (range < 0x100) {
            range <<= 8; low <<= 8;
            if (p < end) low += *p++;
            else ++overread;
        }
        return bit;
    }
};

// the range-coded integer binarisation (RFC 9043 section 3.8.1.2): 32 states per context
inline int get_symbol(RacDec& c, uint8_t* state, bool is_signed, bool* bad = nullptr)
{
    if (c.get(state + 0)) return 0;
    int e = 0;
    while (c.get(state + 1 + std::min(e, 9))) {
        if (++e > 31) { if (bad) *bad = true; return 0; }
    }
    unsigned a = 1;
    for (int i = e - 1; i >= 0; --i) a += a + (unsigned)c.get(state + 22 + std::min(i, 9));
    const int neg = (is_signed && c.get(state + 11 + std::min(e, 10))) ? -1 : 0;
    return (int)((a ^ (unsigned)neg) - (unsigned)neg);
}

struct RacEnc {
    std::vector<uint8_t> out;           // storage; [0, size()) is the stream so far
    uint8_t* w = nullptr;               // write pointer into `out` (ensure() keeps room ahead of it)
    int low = 0, range = 0xFF00;
    int outstanding_count = 0, outstanding_byte = -1;
    const StateTables* tab = &g_default_states;
    void init() { out.resize(4096); w = out.data(); low = 0; range = 0xFF00; outstanding_count = 0; outstanding_byte = -1; }
    size_t size() const { return (size_t)(w - out.data()); }
    // room for `decisions` more binary decisions: each emits at most one byte, plus the pending run of carry bytes
    void ensure(size_t decisions)
    {
        const size_t used = size(), need = used + decisions + (size_t)outstanding_count + 16;
        if (need > out.size()) { out.resize(std::max(need, out.size() * 2)); w = out.data() + used; }
    }
    void finish() { out.resize(size()); }
    inline void renorm()
    {
        while (range < 0x100) {
            if (outstanding_byte < 0) outstanding_byte = low >> 8;
            else if (low <= 0xFF00) {
                *w++ = (uint8_t)outstanding_byte;
                for (; outstanding_count; --outstanding_count) *w++ = 0xFF;
                outstanding_byte = low >> 8;
            } else if (low >= 0x10000) {
                *w++ = (uint8_t)(outstanding_byte + 1);
                for (; outstanding_count; --outstanding_count) *w++ = 0x00;
                outstanding_byte = (low >> 8) & 0xFF;
            } else ++outstanding_count;
            low = (low & 0xFF) << 8;
            range <<= 8;
        }
    }
    inline void put(uint8_t* state, int bit)
    {
        const int range1 = (range * (*state)) >> 8;
        if (!bit) { range -= range1; *state = tab->zero[*state]; }
        else { low += range - range1; range = range1; *state = tab->one[*state]; }
        renorm();
    }
    // FFmpeg's ff_rac_terminate(c, 1): a last bit with state 129 (the sentinel a Golomb-Rice decoder reads; harmless otherwise), flush
    void terminate(bool sentinel)
    {
        ensure(64);
        if (sentinel) { uint8_t st = 129; put(&st, 0); }
        range = 0xFF; low += 0xFF; renorm();
        range = 0xFF; renorm();
        finish();
    }
};

inline void put_symbol(RacEnc& c, uint8_t* state, int v, bool is_signed)
{
    if (!v) { c.put(state + 0, 1); return; }
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    int e = 31;
    while (!(a >> e)) --e;
    c.put(state + 0, 0);
    for (int i = 0; i < e; ++i) c.put(state + 1 + std::min(i, 9), 1);
    c.put(state + 1 + std::min(e, 9), 0);
    for (int i = e - 1; i >= 0; --i) c.put(state + 22 + std::min(i, 9), (int)((a >> i) & 1u));
    if (is_signed) c.put(state + 11 + std::min(e, 10), v < 0);
}

// ---------------------------------------------------------------------------------------------------------------------
// Golomb-Rice side (decoder only; RFC 9043 section 3.8.2)
// ---------------------------------------------------------------------------------------------------------------------
struct BitReader {
    const uint8_t* buf = nullptr; size_t bits = 0, pos = 0;
    void init(const uint8_t* b, size_t bytes) { buf = b; bits = bytes * 8; pos = 0; }
    inline unsigned get1()
    {
        if (pos >= bits) { ++pos; return 0; }
        const unsigned v = (buf[pos >> 3] >> (7 - (pos & 7))) & 1u;
        ++pos;
        return v;
    }
    inline unsigned get(int n) { unsigned v = 0; for (int i = 0; i < n; ++i) v = (v << 1) | get1(); return v; }
};

struct VlcState { int16_t drift = 0; uint16_t error_sum = 4; int8_t bias = 0; uint8_t count = 1; };

inline int fold(int diff, int bits) { const int m = 1 << (bits - 1); return ((diff + m) & ((1 << bits) - 1)) - m; }

// get_ur_golomb(k, limit 12, esc_len): q zeros + a one + k bits -> (q << k) | bits; `limit` zeros -> esc_len bits + limit - 1
inline int get_sr_golomb(BitReader& gb, int k, int esc_len)
{
    int q = 0;
    unsigned v;
    while (q < 12 && !gb.get1()) ++q;
    if (q < 12) v = ((unsigned)q << k) | (k ? gb.get(k) : 0u);
    else v = gb.get(esc_len) + 11u;
    return (int)(v >> 1) ^ -(int)(v & 1u);
}

inline int get_vlc_symbol(BitReader& gb, VlcState& st, int bits)
{
    int i = st.count, k = 0;
    while (i < st.error_sum) { ++k; i += i; }
    int v = get_sr_golomb(gb, k, bits);
    v ^= ((2 * st.drift + st.count) >> 31);
    const int ret = fold(v + st.bias, bits);
    // update_vlc_state
    int drift = st.drift, count = st.count;
    int es = st.error_sum + (v < 0 ? -v : v);
    drift += v;
    if (count == 128) { count >>= 1; drift >>= 1; es >>= 1; }
    ++count;
    if (drift <= -count) { st.bias = (int8_t)std::max(st.bias - 1, -128); drift = std::max(drift + count, -count + 1); }
    else if (drift > 0) { st.bias = (int8_t)std::min(st.bias + 1, 127); drift = std::min(drift - count, 0); }
    st.drift = (int16_t)drift; st.count = (uint8_t)count; st.error_sum = (uint16_t)es;
    return ret;
}

const uint8_t kLog2Run[41] = { 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7,
                               8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24 };

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
    StateTables states;                                        // of the slices' range coders
    bool custom_states = false;
    int plane_count() const { return 2 + alpha; }              // Y, the two chroma planes share one context set, alpha
    bool ycbcr() const { return colorspace == 0; }
    int pix_fmt() const { return !ycbcr() ? MDVT_VIDEO_PIX_RGB : vshift ? MDVT_VIDEO_PIX_YUV420P : hshift ? MDVT_VIDEO_PIX_YUV422P : MDVT_VIDEO_PIX_YUV444P; }
};

// one set of five tables, run-length coded (RFC 9043 section 4.9.? QuantizationTable)
bool read_quant_table(RacDec& c, int16_t* q, int scale, int* levels)
{
    uint8_t state[kContextSize];
    memset(state, 128, sizeof state);
    int i = 0, v = 0;
    for (; i < 128; ++v) {
        bool bad = false;
        const unsigned len = (unsigned)get_symbol(c, state, false, &bad) + 1u;
        if (bad || len > (unsigned)(128 - i)) return false;
        for (unsigned k = 0; k < len; ++k) q[i++] = (int16_t)(scale * v);
    }
    for (i = 1; i < 128; ++i) q[256 - i] = (int16_t)-q[i];
    q[128] = (int16_t)-q[127];
    *levels = 2 * v - 1;
    return true;
}

int read_quant_tables(RacDec& c, int16_t q[kMaxContextInputs][256])
{
    int scale = 1;
    for (int i = 0; i < kMaxContextInputs; ++i) {
        int levels;
        if (!read_quant_table(c, q[i], scale, &levels)) return -1;
        scale *= levels;
        if (scale > 32768 || scale <= 0) return -1;
    }
    return (scale + 1) / 2;
}

void write_quant_table(RacEnc& c, const int16_t* q)
{
    uint8_t state[kContextSize];
    memset(state, 128, sizeof state);
    int last = 0, i;
    for (i = 1; i < 128; ++i)
        if (q[i] != q[i - 1]) { put_symbol(c, state, i - last - 1, false); last = i; }
    put_symbol(c, state, i - last - 1, false);
}

// the configuration record (RFC 9043 section 4.2); for versions 0 / 1 the same fields sit inside the key frame (read_frame_header)
int parse_config_record(const uint8_t* data, size_t size, Ffv1Config& f)
{
    if (size < 6) return fail(ERR_FORMAT, "FFV1 configuration record of %zu bytes", size);
    RacDec c;
    c.init(data, size);
    uint8_t state[kContextSize], state2[kContextSize];
    memset(state, 128, sizeof state);
    memset(state2, 128, sizeof state2);
    bool bad = false;
    f.version = get_symbol(c, state, false, &bad);
    if (f.version > 2) { c.end -= 4; f.micro = get_symbol(c, state, false, &bad); }
    f.coder = get_symbol(c, state, false, &bad);
    if (f.coder == 2) {
        uint8_t one[256];
        one[0] = 0;
        for (int i = 1; i < 256; ++i) one[i] = (uint8_t)(get_symbol(c, state2, true, &bad) + g_default_states.one[i]);
        tables_from_one_state(f.states, one);
        f.custom_states = true;
    } else f.states = g_default_states;
    f.colorspace = get_symbol(c, state, false, &bad);
    f.bits = get_symbol(c, state, false, &bad);
    f.chroma_planes = c.get(state);
    f.hshift = get_symbol(c, state, false, &bad);
    f.vshift = get_symbol(c, state, false, &bad);
    f.alpha = c.get(state);
    f.nh = 1 + get_symbol(c, state, false, &bad);
    f.nv = 1 + get_symbol(c, state, false, &bad);
    f.qcount = get_symbol(c, state, false, &bad);
    if (bad || f.qcount < 1 || f.qcount > kMaxQuantTables || f.nh < 1 || f.nv < 1 || f.nh * f.nv > 4096)
        return fail(ERR_FORMAT, "FFV1 configuration record: bad slice / table counts");
    for (int i = 0; i < f.qcount; ++i) {
        f.context_count[i] = read_quant_tables(c, f.quant[i]);
        if (f.context_count[i] < 0) return fail(ERR_FORMAT, "FFV1 configuration record: bad quantisation table");
    }
    for (int i = 0; i < f.qcount; ++i) {
        f.initial_states[i].clear();
        if (c.get(state)) {
            f.initial_states[i].resize((size_t)f.context_count[i] * kContextSize);
            for (int j = 0; j < f.context_count[i]; ++j)
                for (int k = 0; k < kContextSize; ++k) {
                    const int pred = j ? f.initial_states[i][(size_t)(j - 1) * kContextSize + k] : 128;
                    f.initial_states[i][(size_t)j * kContextSize + k] = (uint8_t)((pred + get_symbol(c, state2, true, &bad)) & 0xFF);
                }
        }
    }
    if (f.version > 2) {
        f.ec = get_symbol(c, state, false, &bad);
        if (f.micro > 2) f.intra = get_symbol(c, state, false, &bad);
        if (crc32_msb(0, data, size) != 0) return fail(ERR_DATA, "FFV1 configuration record: CRC mismatch");
    }
    if (bad) return fail(ERR_FORMAT, "FFV1 configuration record: malformed symbol");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// per-slice context state (kept between frames of a non-intra stream) and the line coder
// ---------------------------------------------------------------------------------------------------------------------
struct PlaneState { int qidx = 0; std::vector<uint8_t> state; std::vector<VlcState> vlc; };
struct SliceState { PlaneState plane[3]; };

void reset_plane(const Ffv1Config& f, PlaneState& p)
{
    const int n = f.context_count[p.qidx];
    if (f.coder) {
        if (!f.initial_states[p.qidx].empty()) p.state = f.initial_states[p.qidx];
        else p.state.assign((size_t)n * kContextSize, 128);
    } else p.vlc.assign((size_t)n, VlcState());
}

inline int median3(int a, int b, int c) { return a > b ? (b > c ? b : (a > c ? c : a)) : (a > c ? a : (b > c ? c : b)); }

// Y, Cb, Cr -> the bytes o[ri], o[1], o[bi]: BT.601 limited range in the integers include/mdvt_video.h states (a decree of this
// project's, not a claim about swscale's bits)
inline uint8_t clip8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
inline void store_ycbcr_pixel(int y, int u, int v, uint8_t* o, int ri, int bi)
{
    const int c = y - 16, d = u - 128, e = v - 128;
    o[ri] = clip8((298 * c + 409 * e + 128) >> 8);
    o[1] = clip8((298 * c - 100 * d - 208 * e + 128) >> 8);
    o[bi] = clip8((298 * c + 516 * d + 128) >> 8);
}

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

struct SliceDecoder {
    const Ffv1Config* f;
    RacDec c;
    BitReader gb;
    int run_index = 0;
    bool error = false;

    // sample[0] = previous line, sample[1] = the line being decoded (still holding the line two rows up: that is TT)
    void decode_line(PlaneState& p, int w, int16_t* sample[2], int bits)
    {
        LineCtx lc{f->quant[p.qidx], f->quant[p.qidx][3][127] != 0 || f->quant[p.qidx][4][127] != 0};
        int run_count = 0, run_mode = 0;
        const int mask = (1 << bits) - 1;
        for (int x = 0; x < w; ++x) {
            int context = get_context(lc, sample[1] + x, sample[0] + x, sample[1] + x);
            const bool sign = context < 0;
            if (sign) context = -context;
            int diff;
            if (f->coder) {
                bool bad = false;
                diff = get_symbol(c, &p.state[(size_t)context * kContextSize], true, &bad);
                error |= bad;
            } else {
                if (context == 0 && run_mode == 0) run_mode = 1;
                if (run_mode) {
                    if (run_count == 0 && run_mode == 1) {
                        if (gb.get1()) {
                            run_count = 1 << kLog2Run[run_index];
                            if (x + run_count <= w) ++run_index;
                        } else {
                            run_count = kLog2Run[run_index] ? (int)gb.get(kLog2Run[run_index]) : 0;
                            if (run_index) --run_index;
                            run_mode = 2;
                        }
                    }
                    --run_count;
                    if (run_count < 0) {
                        run_mode = 0; run_count = 0;
                        diff = get_vlc_symbol(gb, p.vlc[(size_t)context], bits);
                        if (diff >= 0) ++diff;
                    } else diff = 0;
                } else diff = get_vlc_symbol(gb, p.vlc[(size_t)context], bits);
            }
            if (sign) diff = -diff;
            const int pred = median3(sample[1][x - 1], sample[0][x], sample[1][x - 1] + sample[0][x] - sample[0][x - 1]);
            sample[1][x] = (int16_t)((pred + diff) & mask);
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// decoder
// ---------------------------------------------------------------------------------------------------------------------
struct Decoder {
    Ffv1Config f;
    int W = 0, H = 0;
    bool have_config = false;          // version >= 2: from the container; versions 0 / 1: from the first key frame
    bool key_frame_ok = false;
    std::vector<SliceState> slices;

    int read_frame_header(RacDec& c, uint8_t* state)          // versions 0 / 1 (RFC 9043 section 4.? "Frame" with version <= 1)
    {
        bool bad = false;
        const int v = get_symbol(c, state, false, &bad);
        if (bad || v > 1) return fail(ERR_UNSUPPORTED, "FFV1 frame header announces version %d inside the frame", v);
        f.version = v;
        f.coder = get_symbol(c, state, false, &bad);
        if (f.coder == 2) {
            uint8_t one[256];
            one[0] = 0;
            for (int i = 1; i < 256; ++i) one[i] = (uint8_t)(get_symbol(c, state, true, &bad) + g_default_states.one[i]);
            tables_from_one_state(f.states, one);
            f.custom_states = true;
        } else f.states = g_default_states;
        f.colorspace = get_symbol(c, state, false, &bad);
        f.bits = f.version > 0 ? get_symbol(c, state, false, &bad) : 8;
        f.chroma_planes = c.get(state);
        f.hshift = get_symbol(c, state, false, &bad);
        f.vshift = get_symbol(c, state, false, &bad);
        f.alpha = c.get(state);
        f.nh = f.nv = 1; f.qcount = 1; f.ec = 0; f.intra = 0;
        f.context_count[0] = read_quant_tables(c, f.quant[0]);
        if (bad || f.context_count[0] < 0) return fail(ERR_FORMAT, "FFV1 frame header: malformed");
        f.initial_states[0].clear();
        return 0;
    }

    int check_supported() const
    {
        if (f.version != 0 && f.version != 1 && f.version != 3)
            return fail(ERR_UNSUPPORTED, "FFV1 version %d (0, 1 and 3 are implemented; 2 was experimental, 4 is not final)", f.version);
        if (f.colorspace != 0 && f.colorspace != 1)
            return fail(ERR_UNSUPPORTED, "FFV1 colorspace_type %d: YCbCr (0) and RGB (1, the JPEG 2000 RCT) are implemented", f.colorspace);
        if (f.bits != 0 && f.bits != 8) return fail(ERR_UNSUPPORTED, "FFV1 with %d bits per sample (8 implemented)", f.bits);
        if (f.coder < 0 || f.coder > 2) return fail(ERR_FORMAT, "FFV1 coder_type %d", f.coder);
        if (!f.ycbcr()) return 0;
        if (f.alpha) return fail(ERR_UNSUPPORTED, "FFV1 YCbCr with an alpha plane (extra_plane 1) is not implemented");
        if (!f.chroma_planes) return fail(ERR_UNSUPPORTED, "FFV1 YCbCr with chroma_planes 0 (grey) is not implemented");
        const int hs = f.hshift, vs = f.vshift;
        if (!((hs == 0 && vs == 0) || (hs == 1 && vs == 0) || (hs == 1 && vs == 1)))
            return fail(ERR_UNSUPPORTED, "FFV1 YCbCr with chroma subsampling shifts (%d, %d): (0, 0), (1, 0) and (1, 1) -- yuv444p, yuv422p, "
                                         "yuv420p -- are implemented", hs, vs);
        // a slice's chroma rectangle starts at (x0 >> hs, y0 >> vs): the chroma rectangles tile the chroma plane only when every
        // slice origin is a multiple of the subsampling
        if (f.version >= 3) {
            for (int sx = 0; sx < f.nh; ++sx)
                if (((int64_t)sx * W / f.nh) & ((1 << hs) - 1))
                    return fail(ERR_UNSUPPORTED, "FFV1 YCbCr: the %d x %d slice grid puts a slice at x = %d of the %d x %d frame, off the chroma "
                                                 "grid of shifts (%d, %d); only aligned slice grids are decoded", f.nh, f.nv,
                                (int)((int64_t)sx * W / f.nh), W, H, hs, vs);
            for (int sy = 0; sy < f.nv; ++sy)
                if (((int64_t)sy * H / f.nv) & ((1 << vs) - 1))
                    return fail(ERR_UNSUPPORTED, "FFV1 YCbCr: the %d x %d slice grid puts a slice at y = %d of the %d x %d frame, off the chroma "
                                                 "grid of shifts (%d, %d); only aligned slice grids are decoded", f.nh, f.nv,
                                (int)((int64_t)sy * H / f.nv), W, H, hs, vs);
        }
        return 0;
    }

    // one slice: [start, start + size) of the packet is its range-coded / Golomb-coded payload (trailer already cut off)
    int decode_slice(int index, const uint8_t* data, size_t size, bool first, bool key, uint8_t* dst, size_t pitch, int order, RacDec* started)
    {
        SliceDecoder sd;
        sd.f = &f;
        if (started) sd.c = *started;
        else if (!sd.c.init(data, size)) return fail(ERR_DATA, "FFV1 slice %d: %zu bytes", index, size);
        sd.c.tab = &f.states;
        if (started) sd.c.end = data + size;
        SliceState& ss = slices[(size_t)index];
        int x0 = 0, y0 = 0, sw = W, sh = H;
        if (f.version >= 3) {
            uint8_t state[kContextSize];
            memset(state, 128, sizeof state);
            bool bad = false;
            const unsigned sx = (unsigned)get_symbol(sd.c, state, false, &bad), sy = (unsigned)get_symbol(sd.c, state, false, &bad);
            const unsigned cw = (unsigned)get_symbol(sd.c, state, false, &bad) + 1u, ch = (unsigned)get_symbol(sd.c, state, false, &bad) + 1u;
            if (bad || sx >= (unsigned)f.nh || sy >= (unsigned)f.nv || sx + cw > (unsigned)f.nh || sy + ch > (unsigned)f.nv)
                return fail(ERR_DATA, "FFV1 slice %d: bad slice position", index);
            x0 = (int)((int64_t)sx * W / f.nh); y0 = (int)((int64_t)sy * H / f.nv);
            sw = (int)((int64_t)(sx + cw) * W / f.nh) - x0; sh = (int)((int64_t)(sy + ch) * H / f.nv) - y0;
            for (int p = 0; p < f.plane_count(); ++p) {
                const int idx = get_symbol(sd.c, state, false, &bad);
                if (bad || idx < 0 || idx >= f.qcount) return fail(ERR_DATA, "FFV1 slice %d: bad quantisation table index", index);
                if (ss.plane[p].qidx != idx) { ss.plane[p].qidx = idx; ss.plane[p].state.clear(); ss.plane[p].vlc.clear(); }
            }
            (void)get_symbol(sd.c, state, false, &bad);      // picture_structure
            (void)get_symbol(sd.c, state, false, &bad);      // sar_num
            (void)get_symbol(sd.c, state, false, &bad);      // sar_den
            if (bad) return fail(ERR_DATA, "FFV1 slice %d: malformed header", index);
        }
        for (int p = 0; p < f.plane_count(); ++p) {
            PlaneState& ps = ss.plane[p];
            const bool empty = f.coder ? ps.state.empty() : ps.vlc.empty();
            if (key || empty) {
                if (!key && empty) return fail(ERR_DATA, "FFV1: inter frame without a preceding key frame");
                reset_plane(f, ps);
            }
        }
        if (f.coder == 0) {
            if ((f.version == 3 && f.micro > 1) || f.version > 3) { uint8_t st = 129; (void)sd.c.get(&st); }
            const size_t consumed = (size_t)(sd.c.p - sd.c.start) - 1;
            const uint8_t* base = sd.c.start;
            const size_t total = (size_t)((data + size) - base);
            if (consumed > total) return fail(ERR_DATA, "FFV1 slice %d: header overruns the slice", index);
            sd.gb.init(base + consumed, total - consumed);
        }
        const int ri = order == MDVT_VIDEO_BGR ? 2 : 0, bi = order == MDVT_VIDEO_BGR ? 0 : 2;
        if (f.ycbcr()) {
            // ---- YCbCr: plane after plane, 8-bit samples, the run index restarting at each plane (RFC 9043 section 4.6) ----
            const int hs = f.hshift, vs = f.vshift;
            const int cw = (sw + (1 << hs) - 1) >> hs, chh = (sh + (1 << vs) - 1) >> vs;
            std::vector<uint8_t> pl[3];
            std::vector<int16_t> buf((size_t)2 * (size_t)(sw + 6));
            for (int p = 0; p < 3; ++p) {
                const int w = p ? cw : sw, h = p ? chh : sh;
                pl[p].resize((size_t)w * (size_t)h);
                std::fill(buf.begin(), buf.end(), (int16_t)0);
                int16_t* sample[2] = {buf.data() + 3, buf.data() + (size_t)(sw + 6) + 3};
                sd.run_index = 0;
                for (int y = 0; y < h; ++y) {
                    std::swap(sample[0], sample[1]);
                    sample[1][-1] = sample[0][0];
                    sample[0][w] = sample[0][w - 1];
                    sd.decode_line(ss.plane[p ? 1 : 0], w, sample, 8);
                    for (int x = 0; x < w; ++x) pl[p][(size_t)y * (size_t)w + (size_t)x] = (uint8_t)sample[1][x];
                }
            }
            for (int y = 0; y < sh; ++y) {
                uint8_t* o = dst + (size_t)(y0 + y) * pitch + (size_t)x0 * 3;
                const uint8_t* ly = pl[0].data() + (size_t)y * (size_t)sw;
                const uint8_t* lu = pl[1].data() + (size_t)(y >> vs) * (size_t)cw;
                const uint8_t* lv = pl[2].data() + (size_t)(y >> vs) * (size_t)cw;
                for (int x = 0; x < sw; ++x) store_ycbcr_pixel(ly[x], lu[x >> hs], lv[x >> hs], o + 3 * x, ri, bi);
            }
            if (sd.error || sd.c.overread > 4) return fail(ERR_DATA, "FFV1 slice %d: bitstream damaged (overread %d)", index, sd.c.overread);
            return 0;
        }
        // ---- RGB: lines of Y, Cb, Cr (, A) interleaved (RFC 9043 section 3.7.2 / 4.7) ----
        const int np = 3 + f.alpha;
        std::vector<int16_t> buf((size_t)np * 2 * (size_t)(sw + 6), 0);
        int16_t* sample[4][2];
        for (int p = 0; p < np; ++p)
            for (int k = 0; k < 2; ++k) sample[p][k] = buf.data() + ((size_t)p * 2 + (size_t)k) * (size_t)(sw + 6) + 3;
        sd.run_index = 0;
        for (int y = 0; y < sh; ++y) {
            for (int p = 0; p < np; ++p) {
                std::swap(sample[p][0], sample[p][1]);
                sample[p][1][-1] = sample[p][0][0];
                sample[p][0][sw] = sample[p][0][sw - 1];
                PlaneState& ps = ss.plane[p == 3 ? 2 : (p + 1) / 2];
                sd.decode_line(ps, sw, sample[p], 9);                        // 8-bit RGB: every plane, alpha included, is coded with 9 bits
            }
            uint8_t* o = dst + (size_t)(y0 + y) * pitch + (size_t)x0 * 3;
            for (int x = 0; x < sw; ++x) {
                int g = sample[0][1][x], b = sample[1][1][x] - 256, r = sample[2][1][x] - 256;
                g -= (b + r) >> 2;
                b += g; r += g;
                o[3 * x + ri] = (uint8_t)r; o[3 * x + 1] = (uint8_t)g; o[3 * x + bi] = (uint8_t)b;
            }
        }
        if (sd.error || sd.c.overread > 4) return fail(ERR_DATA, "FFV1 slice %d: bitstream damaged (overread %d)", index, sd.c.overread);
        (void)first;
        return 0;
    }

    int decode_frame(const uint8_t* pkt, size_t size, uint8_t* dst, size_t pitch, int order, int threads)
    {
        if (size < 3) return fail(ERR_DATA, "FFV1 packet of %zu bytes", size);
        RacDec c;
        c.init(pkt, size);
        uint8_t keystate = 128;
        const bool key = c.get(&keystate) != 0;
        if (key) {
            if (!have_config || f.version < 2) {
                uint8_t state[kContextSize];
                memset(state, 128, sizeof state);
                int rc = read_frame_header(c, state);
                if (rc) return rc;
                have_config = true;
            }
            int rc = check_supported();
            if (rc) return rc;
            key_frame_ok = true;
        } else if (!key_frame_ok) return fail(ERR_DATA, "FFV1: the stream does not start with a key frame");
        const int n = f.version >= 3 ? f.nh * f.nv : 1;
        if ((int)slices.size() != n) slices.assign((size_t)n, SliceState());
        // slice extents, from the end of the packet (RFC 9043 section 4.? slice footers)
        std::vector<std::pair<size_t, size_t>> ext((size_t)n);      // offset, payload size
        if (f.version >= 3) {
            const size_t trailer = 3 + (f.ec ? 5 : 0);
            size_t end = size;
            for (int i = n - 1; i >= 0; --i) {
                if (end < trailer) return fail(ERR_DATA, "FFV1: packet too short for %d slices", n);
                const uint8_t* t = pkt + end - trailer;
                const size_t payload = ((size_t)t[0] << 16) | ((size_t)t[1] << 8) | t[2];
                if (payload + trailer > end) return fail(ERR_DATA, "FFV1: slice %d claims %zu bytes", i, payload);
                const size_t off = end - trailer - payload;
                if (f.ec && crc32_msb(0, pkt + off, payload + trailer) != 0) return fail(ERR_DATA, "FFV1: CRC mismatch in slice %d", i);
                ext[(size_t)i] = {off, payload};
                end = off;
            }
            if (end != 0) return fail(ERR_DATA, "FFV1: %zu stray bytes before the first slice", end);
        } else ext[0] = {0, size};
        std::atomic<int> next(0), failed(0);
        std::string err;
        auto work = [&]() {
            for (;;) {
                const int i = next.fetch_add(1);
                if (i >= n) break;
                const int rc = decode_slice(i, pkt + ext[(size_t)i].first, ext[(size_t)i].second, i == 0, key, dst, pitch, order, i == 0 ? &c : nullptr);
                if (rc) { failed = rc; }
            }
        };
        int nt = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
        nt = std::max(1, std::min(nt, n));
        if (nt == 1) work();
        else {
            std::vector<std::thread> th;
            std::vector<std::string> errs((size_t)nt);
            for (int t = 0; t < nt; ++t) th.emplace_back([&, t]() { work(); errs[(size_t)t] = g_err; });
            for (auto& t : th) t.join();
            if (failed) for (auto& e : errs) if (!e.empty()) g_err = e;
        }
        return failed;
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// encoder: version 3.4, range coder with the default table, intra-only, RGB, 8 bits
// ---------------------------------------------------------------------------------------------------------------------
// FFmpeg's quant11 (ffv1enc.c): the 11-level quantisation of a sample difference used for 8-bit input, context model 0
int quant11_of(int i)      // i in 0..255 as an index = (difference & 0xFF)
{
    const int d = i < 128 ? i : i - 256;
    const int a = d < 0 ? -d : d;
    int q = a == 0 ? 0 : a < 2 ? 1 : a < 5 ? 2 : a < 12 ? 3 : a < 32 ? 4 : 5;
    if (i == 128) q = 5;
    return d < 0 ? -q : q;
}

struct EncoderTables {
    int16_t q[kMaxContextInputs][256];
    int context_count;
    EncoderTables()
    {
        for (int i = 0; i < 256; ++i) {
            q[0][i] = (int16_t)quant11_of(i);
            q[1][i] = (int16_t)(11 * quant11_of(i));
            q[2][i] = (int16_t)(11 * 11 * quant11_of(i));
            q[3][i] = q[4][i] = 0;
        }
        context_count = (11 * 11 * 11 + 1) / 2;
    }
};
const EncoderTables g_enc_tables;

// (colorspace 0 with its chroma shifts: tools/ffv1_ycbcr_writer.cpp, which makes YCbCr streams for measurements; no writer of this library's does)
std::vector<uint8_t> make_config_record(int nh, int nv, int coder = 1, int intra = 1, int colorspace = 1, int hshift = 0, int vshift = 0)
{
    RacEnc c;
    c.init();
    c.ensure(8192);
    uint8_t state[kContextSize];
    memset(state, 128, sizeof state);
    put_symbol(c, state, 3, false);          // version
    put_symbol(c, state, 4, false);          // micro_version
    put_symbol(c, state, coder, false);      // coder_type: 1 range coder, default state transition table; 0 Golomb-Rice (the stream class)
    put_symbol(c, state, colorspace, false); // colorspace_type: RGB
    put_symbol(c, state, 8, false);          // bits_per_raw_sample
    c.put(state, 1);                         // chroma_planes
    put_symbol(c, state, hshift, false);     // log2_h_chroma_subsample
    put_symbol(c, state, vshift, false);     // log2_v_chroma_subsample
    c.put(state, 0);                         // extra_plane
    put_symbol(c, state, nh - 1, false);
    put_symbol(c, state, nv - 1, false);
    put_symbol(c, state, 1, false);          // quant_table_set_count
    for (int i = 0; i < kMaxContextInputs; ++i) write_quant_table(c, g_enc_tables.q[i]);
    c.put(state, 0);                         // states_coded
    put_symbol(c, state, 1, false);          // ec
    put_symbol(c, state, intra, false);      // intra
    c.terminate(false);
    std::vector<uint8_t> out = c.out;
    const uint32_t crc = crc32_msb(0, out.data(), out.size());
    out.push_back((uint8_t)(crc >> 24)); out.push_back((uint8_t)(crc >> 16)); out.push_back((uint8_t)(crc >> 8)); out.push_back((uint8_t)crc);
    return out;
}

void encode_slice(int W, int H, int nh, int nv, int sx, int sy, const uint8_t* src, size_t pitch, int order, bool first, std::vector<uint8_t>& out)
{
    const int x0 = (int)((int64_t)sx * W / nh), y0 = (int)((int64_t)sy * H / nv);
    const int sw = (int)((int64_t)(sx + 1) * W / nh) - x0, sh = (int)((int64_t)(sy + 1) * H / nv) - y0;
    RacEnc c;
    c.init();
    c.ensure(1024);
    if (first) { uint8_t keystate = 128; c.put(&keystate, 1); }       // every frame is a key frame
    uint8_t hstate[kContextSize];
    memset(hstate, 128, sizeof hstate);
    put_symbol(c, hstate, sx, false);
    put_symbol(c, hstate, sy, false);
    put_symbol(c, hstate, 0, false);         // slice_width - 1 (in slice units)
    put_symbol(c, hstate, 0, false);
    put_symbol(c, hstate, 0, false);         // quant_table_set_index of the luma plane ...
    put_symbol(c, hstate, 0, false);         // ... and of the chroma planes
    put_symbol(c, hstate, 3, false);         // picture_structure: progressive
    put_symbol(c, hstate, 0, false);         // sar_num
    put_symbol(c, hstate, 0, false);         // sar_den: unknown
    std::vector<uint8_t> st[2];
    st[0].assign((size_t)g_enc_tables.context_count * kContextSize, 128);
    st[1].assign((size_t)g_enc_tables.context_count * kContextSize, 128);
    std::vector<int16_t> buf((size_t)3 * 2 * (size_t)(sw + 6), 0);
    int16_t* sample[3][2];
    for (int p = 0; p < 3; ++p)
        for (int k = 0; k < 2; ++k) sample[p][k] = buf.data() + ((size_t)p * 2 + (size_t)k) * (size_t)(sw + 6) + 3;
    const int ri = order == MDVT_VIDEO_BGR ? 2 : 0, bi = order == MDVT_VIDEO_BGR ? 0 : 2;
    LineCtx lc{g_enc_tables.q, false};
    for (int y = 0; y < sh; ++y) {
        const uint8_t* s = src + (size_t)(y0 + y) * pitch + (size_t)x0 * 3;
        for (int p = 0; p < 3; ++p) std::swap(sample[p][0], sample[p][1]);         // [0] = previous line, [1] = this line
        for (int x = 0; x < sw; ++x) {
            int r = s[3 * x + ri], g = s[3 * x + 1], b = s[3 * x + bi];
            b -= g; r -= g;
            g += (b + r) >> 2;
            sample[0][1][x] = (int16_t)g; sample[1][1][x] = (int16_t)(b + 256); sample[2][1][x] = (int16_t)(r + 256);
        }
        c.ensure((size_t)sw * 3 * 24);          // a sample is at most 23 binary decisions
        for (int p = 0; p < 3; ++p) {
            int16_t* cur = sample[p][1];
            int16_t* last = sample[p][0];
            cur[-1] = last[0];
            last[sw] = last[sw - 1];
            uint8_t* states = st[(p + 1) / 2].data();
            for (int x = 0; x < sw; ++x) {
                int context = get_context(lc, cur + x, last + x, cur + x);
                int diff = cur[x] - median3(cur[x - 1], last[x], cur[x - 1] + last[x] - last[x - 1]);
                if (context < 0) { context = -context; diff = -diff; }
                diff = fold(diff, 9);
                put_symbol(c, states + (size_t)context * kContextSize, diff, true);
            }
        }
    }
    c.terminate(true);
    out = c.out;
    const size_t payload = out.size();
    out.push_back((uint8_t)(payload >> 16)); out.push_back((uint8_t)(payload >> 8)); out.push_back((uint8_t)payload);
    out.push_back(0);                                                                 // error_status
    const uint32_t crc = crc32_msb(0, out.data(), out.size());
    out.push_back((uint8_t)(crc >> 24)); out.push_back((uint8_t)(crc >> 16)); out.push_back((uint8_t)(crc >> 8)); out.push_back((uint8_t)crc);
}

int encode_frame(int W, int H, int nh, int nv, const uint8_t* src, size_t pitch, int order, int threads, std::vector<uint8_t>& packet)
{
    const int n = nh * nv;
    std::vector<std::vector<uint8_t>> parts((size_t)n);
    std::atomic<int> next(0);
    auto work = [&]() {
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= n) break;
            encode_slice(W, H, nh, nv, i % nh, i / nh, src, pitch, order, i == 0, parts[(size_t)i]);
        }
    };
    int nt = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    nt = std::max(1, std::min(nt, n));
    if (nt == 1) work();
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t) th.emplace_back(work);
        for (auto& t : th) t.join();
    }
    size_t total = 0;
    for (auto& p : parts) total += p.size();
    packet.clear();
    packet.reserve(total);
    for (auto& p : parts) {
        if (p.size() - 8 >= (1u << 24)) return fail(ERR_UNSUPPORTED, "an FFV1 slice of %zu bytes does not fit the 24-bit slice size: use more slices", p.size());
        packet.insert(packet.end(), p.begin(), p.end());
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// encoder of the opt-in stream class (include/mdvt_video_stream.h): version 3.4, Golomb-Rice with run mode, intra = 0, a key frame
// every `gop` frames, CRC-32 parities -- what FFmpeg writes by default for 8-bit RGB.  A slice's VLC states carry from frame to
// frame and are reset at a key frame.  Byte for byte the independent restatement ffv1_ref.py's StreamEncoder(Params(coder=0, intra=0, nh, nv), W, H, gop).
// ---------------------------------------------------------------------------------------------------------------------
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

struct GolombSliceState { std::vector<VlcState> vlc[2]; };

inline void put_vlc_symbol(BitWriter& bw, VlcState& st, int diff, int bits = 9)
{
    const int v = fold(diff - st.bias, bits);
    int i = st.count, k = 0;
    while (i < st.error_sum) { ++k; i += i; }
    const int code = v ^ ((2 * st.drift + st.count) >> 31);
    const unsigned u = code >= 0 ? 2u * (unsigned)code : 2u * (unsigned)(-code) - 1u;
    if ((u >> k) < 12u) bw.put((int)(u >> k) + k + 1, (1u << k) + (u & ((1u << k) - 1u)));
    else bw.put(12 + bits, u - 11u);
    // update_vlc_state, as get_vlc_symbol does it
    int drift = st.drift + v, count = st.count;
    int es = st.error_sum + (v < 0 ? -v : v);
    if (count == 128) { count >>= 1; drift >>= 1; es >>= 1; }
    ++count;
    if (drift <= -count) { st.bias = (int8_t)std::max(st.bias - 1, -128); drift = std::max(drift + count, -count + 1); }
    else if (drift > 0) { st.bias = (int8_t)std::min(st.bias + 1, 127); drift = std::min(drift - count, 0); }
    st.drift = (int16_t)drift; st.count = (uint8_t)count; st.error_sum = (uint16_t)es;
}

void encode_slice_golomb(int W, int H, int nh, int nv, int sx, int sy, const uint8_t* src, size_t pitch, int order, bool first, bool key,
                         GolombSliceState& ss, std::vector<uint8_t>& out)
{
    const int x0 = (int)((int64_t)sx * W / nh), y0 = (int)((int64_t)sy * H / nv);
    const int sw = (int)((int64_t)(sx + 1) * W / nh) - x0, sh = (int)((int64_t)(sy + 1) * H / nv) - y0;
    RacEnc c;
    c.init();
    c.ensure(1024);
    if (first) { uint8_t keystate = 128; c.put(&keystate, key ? 1 : 0); }
    uint8_t hstate[kContextSize];
    memset(hstate, 128, sizeof hstate);
    const int header[9] = {sx, sy, 0, 0, 0, 0, 3, 0, 0};        // position, size - 1 in slice units, two table indices, progressive, unknown aspect
    for (int v : header) put_symbol(c, hstate, v, false);
    c.terminate(true);                                          // the sentinel bit: the bit stream starts behind the range coder's bytes
    if (key || ss.vlc[0].empty())
        for (auto& v : ss.vlc) v.assign((size_t)g_enc_tables.context_count, VlcState());
    BitWriter bw;
    bw.out.reserve((size_t)sw * sh * 3);
    std::vector<int16_t> buf((size_t)3 * 2 * (size_t)(sw + 6), 0);
    int16_t* sample[3][2];
    for (int p = 0; p < 3; ++p)
        for (int k = 0; k < 2; ++k) sample[p][k] = buf.data() + ((size_t)p * 2 + (size_t)k) * (size_t)(sw + 6) + 3;
    const int ri = order == MDVT_VIDEO_BGR ? 2 : 0, bi = order == MDVT_VIDEO_BGR ? 0 : 2;
    LineCtx lc{g_enc_tables.q, false};
    int run_index = 0;
    auto flush_run = [&](int& run_count) {                      // whole runs of the current length: a one bit each
        while (run_count >= (1 << kLog2Run[run_index])) { run_count -= 1 << kLog2Run[run_index]; if (run_index < 40) ++run_index; bw.put(1, 1); }
    };
    for (int y = 0; y < sh; ++y) {
        const uint8_t* s = src + (size_t)(y0 + y) * pitch + (size_t)x0 * 3;
        for (int p = 0; p < 3; ++p) std::swap(sample[p][0], sample[p][1]);
        for (int x = 0; x < sw; ++x) {
            int r = s[3 * x + ri], g = s[3 * x + 1], b = s[3 * x + bi];
            b -= g; r -= g;
            g += (b + r) >> 2;
            sample[0][1][x] = (int16_t)g; sample[1][1][x] = (int16_t)(b + 256); sample[2][1][x] = (int16_t)(r + 256);
        }
        for (int p = 0; p < 3; ++p) {
            int16_t* cur = sample[p][1];
            int16_t* last = sample[p][0];
            cur[-1] = last[0];
            last[sw] = last[sw - 1];
            VlcState* vlc = ss.vlc[(p + 1) / 2].data();
            int run_count = 0, run_mode = 0;
            for (int x = 0; x < sw; ++x) {
                int context = get_context(lc, cur + x, last + x, cur + x);
                int diff = cur[x] - median3(cur[x - 1], last[x], cur[x - 1] + last[x] - last[x - 1]);
                if (context < 0) { context = -context; diff = -diff; }
                diff = fold(diff, 9);
                if (context == 0) run_mode = 1;
                if (run_mode) {
                    if (diff) {
                        flush_run(run_count);
                        bw.put(1 + kLog2Run[run_index], (uint32_t)run_count);
                        if (run_index) --run_index;
                        run_count = 0; run_mode = 0;
                        if (diff > 0) --diff;
                    } else ++run_count;
                }
                if (run_mode == 0) put_vlc_symbol(bw, vlc[(size_t)context], diff);
            }
            if (run_mode) {
                flush_run(run_count);
                if (run_count) bw.put(1, 1);
            }
        }
    }
    bw.flush();
    out = c.out;
    out.insert(out.end(), bw.out.begin(), bw.out.end());
    const size_t payload = out.size();
    out.push_back((uint8_t)(payload >> 16)); out.push_back((uint8_t)(payload >> 8)); out.push_back((uint8_t)payload);
    out.push_back(0);                                                                 // error_status
    const uint32_t crc = crc32_msb(0, out.data(), out.size());
    out.push_back((uint8_t)(crc >> 24)); out.push_back((uint8_t)(crc >> 16)); out.push_back((uint8_t)(crc >> 8)); out.push_back((uint8_t)crc);
}

int encode_frame_golomb(int W, int H, int nh, int nv, const uint8_t* src, size_t pitch, int order, int threads, bool key,
                        std::vector<GolombSliceState>& states, std::vector<uint8_t>& packet)
{
    const int n = nh * nv;
    states.resize((size_t)n);
    std::vector<std::vector<uint8_t>> parts((size_t)n);
    std::atomic<int> next(0);
    auto work = [&]() {
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= n) break;
            encode_slice_golomb(W, H, nh, nv, i % nh, i / nh, src, pitch, order, i == 0, key, states[(size_t)i], parts[(size_t)i]);
        }
    };
    int nt = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    nt = std::max(1, std::min(nt, n));
    if (nt == 1) work();
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t) th.emplace_back(work);
        for (auto& t : th) t.join();
    }
    packet.clear();
    for (auto& p : parts) {
        if (p.size() - 8 >= (1u << 24)) return fail(ERR_UNSUPPORTED, "an FFV1 slice of %zu bytes does not fit the 24-bit slice size: use more slices", p.size());
        packet.insert(packet.end(), p.begin(), p.end());
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// EBML / Matroska
// ---------------------------------------------------------------------------------------------------------------------
enum : uint32_t {
    ID_EBML = 0x1A45DFA3, ID_SEGMENT = 0x18538067, ID_INFO = 0x1549A966, ID_TRACKS = 0x1654AE6B, ID_CLUSTER = 0x1F43B675,
    ID_CUES = 0x1C53BB6B, ID_TIMECODESCALE = 0x2AD7B1, ID_DURATION = 0x4489, ID_TRACKENTRY = 0xAE, ID_TRACKNUMBER = 0xD7,
    ID_TRACKTYPE = 0x83, ID_CODECID = 0x86, ID_CODECPRIVATE = 0x63A2, ID_DEFAULTDURATION = 0x23E383, ID_VIDEO = 0xE0,
    ID_PIXELWIDTH = 0xB0, ID_PIXELHEIGHT = 0xBA, ID_TIMECODE = 0xE7, ID_SIMPLEBLOCK = 0xA3, ID_BLOCKGROUP = 0xA0, ID_BLOCK = 0xA1,
    ID_MUXINGAPP = 0x4D80, ID_WRITINGAPP = 0x5741, ID_TRACKUID = 0x73C5, ID_FLAGLACING = 0x9C, ID_CUEPOINT = 0xBB,
    ID_CUETIME = 0xB3, ID_CUETRACKPOSITIONS = 0xB7, ID_CUETRACK = 0xF7, ID_CUECLUSTERPOSITION = 0xF1, ID_DOCTYPE = 0x4282,
    ID_DOCTYPEVERSION = 0x4287, ID_DOCTYPEREADVERSION = 0x4285, ID_EBMLVERSION = 0x4286, ID_EBMLREADVERSION = 0x42F7,
    ID_EBMLMAXIDLENGTH = 0x42F2, ID_EBMLMAXSIZELENGTH = 0x42F3, ID_VOID = 0xEC, ID_SEEKHEAD = 0x114D9B74,
};
constexpr uint64_t kUnknownSize = ~0ull;

struct FileReader {
    FILE* fp = nullptr;
    uint64_t size = 0;
    ~FileReader() { if (fp) fclose(fp); }
    bool open(const char* path)
    {
        fp = fopen(path, "rb");
        if (!fp) return false;
        fseeko(fp, 0, SEEK_END);
        size = (uint64_t)ftello(fp);
        fseeko(fp, 0, SEEK_SET);
        return true;
    }
    bool read_at(uint64_t off, void* dst, size_t n) { return fseeko(fp, (off_t)off, SEEK_SET) == 0 && fread(dst, 1, n, fp) == n; }
};

// element id (with its marker bits) and data size at `off`; returns the header length or 0
int read_element_header(FileReader& f, uint64_t off, uint32_t* id, uint64_t* size)
{
    uint8_t b[12];
    const size_t avail = (size_t)std::min<uint64_t>(12, f.size > off ? f.size - off : 0);
    if (avail < 2 || !f.read_at(off, b, avail)) return 0;
    int idlen = 1;
    while (idlen <= 4 && !(b[0] & (0x80 >> (idlen - 1)))) ++idlen;
    if (idlen > 4 || (size_t)idlen >= avail) return 0;
    uint32_t v = 0;
    for (int i = 0; i < idlen; ++i) v = (v << 8) | b[i];
    int slen = 1;
    while (slen <= 8 && !(b[idlen] & (0x80 >> (slen - 1)))) ++slen;
    if (slen > 8 || (size_t)(idlen + slen) > avail) return 0;
    uint64_t s = b[idlen] & (0xFFu >> slen);
    bool all_ones = s == (0xFFu >> slen);
    for (int i = 1; i < slen; ++i) { s = (s << 8) | b[idlen + i]; all_ones &= b[idlen + i] == 0xFF; }
    *id = v;
    *size = all_ones ? kUnknownSize : s;
    return idlen + slen;
}

uint64_t read_uint(FileReader& f, uint64_t off, uint64_t size)
{
    uint8_t b[8] = {0};
    if (size > 8 || !f.read_at(off, b, (size_t)size)) return 0;
    uint64_t v = 0;
    for (uint64_t i = 0; i < size; ++i) v = (v << 8) | b[i];
    return v;
}

double read_float(FileReader& f, uint64_t off, uint64_t size)
{
    if (size == 4) { uint32_t u = (uint32_t)read_uint(f, off, 4); float x; memcpy(&x, &u, 4); return x; }
    if (size == 8) { uint64_t u = read_uint(f, off, 8); double x; memcpy(&x, &u, 8); return x; }
    return 0.0;
}

struct FrameRef { uint64_t offset; uint32_t size; int64_t timecode; };

}  // namespace

struct mdvt_video_reader {
    FileReader file;
    Decoder dec;
    std::vector<FrameRef> frames;
    size_t next = 0;
    std::vector<uint8_t> packet;
    std::vector<uint8_t> config;
    mdvt_video_info info{};
};

namespace {

// walks the children of a master element [off, end)
template <class F>
bool for_children(FileReader& f, uint64_t off, uint64_t end, F&& fn)
{
    while (off < end) {
        uint32_t id; uint64_t size;
        const int h = read_element_header(f, off, &id, &size);
        if (!h) return false;
        uint64_t data = off + (uint64_t)h;
        if (size == kUnknownSize) size = end - data;          // (only Segment / Cluster may be unknown-sized: runs to the parent's end)
        if (data + size > end) size = end - data;             // a truncated file: take what is there
        if (!fn(id, data, size)) return false;
        off = data + size;
    }
    return true;
}

int index_matroska(mdvt_video_reader& r)
{
    FileReader& f = r.file;
    uint32_t id; uint64_t size;
    int h = read_element_header(f, 0, &id, &size);
    if (!h || id != ID_EBML) return fail(ERR_FORMAT, "not a Matroska file (no EBML header)");
    uint64_t off = (uint64_t)h + size;
    h = read_element_header(f, off, &id, &size);
    while (h && id != ID_SEGMENT) { off += (uint64_t)h + size; h = read_element_header(f, off, &id, &size); }
    if (!h) return fail(ERR_FORMAT, "Matroska: no Segment");
    const uint64_t seg = off + (uint64_t)h, seg_end = size == kUnknownSize ? f.size : std::min(f.size, seg + size);
    uint64_t timecode_scale = 1000000, default_duration = 0;
    double duration = 0.0;
    int track = -1;
    std::vector<uint8_t> priv;
    std::string codec;
    int pw = 0, ph = 0;
    // A Cluster of unknown size (a muxer that could not seek) runs, for this walk, to the end of the Segment: the Clusters that
    // follow then show up as its children and are walked as Clusters in their own right.
    std::function<void(uint64_t, uint64_t)> walk_cluster = [&](uint64_t d1, uint64_t s1) {
        int64_t cluster_tc = 0;
        for_children(f, d1, d1 + s1, [&](uint32_t id2, uint64_t d2, uint64_t s2) {
            if (id2 == ID_TIMECODE) cluster_tc = (int64_t)read_uint(f, d2, s2);
            auto block = [&](uint64_t d, uint64_t s) {
                uint8_t b[4];
                if (s < 4 || !f.read_at(d, b, 4)) return;
                if (!(b[0] & 0x80)) return;                             // track numbers above 127: not ours
                const int tn = b[0] & 0x7F;
                const int16_t rel = (int16_t)((b[1] << 8) | b[2]);
                if (b[3] & 0x06) return;                                // laced blocks: not video
                if (tn == track) r.frames.push_back({d + 4, (uint32_t)(s - 4), cluster_tc + rel});
            };
            if (id2 == ID_SIMPLEBLOCK) block(d2, s2);
            else if (id2 == ID_BLOCKGROUP)
                for_children(f, d2, d2 + s2, [&](uint32_t id3, uint64_t d3, uint64_t s3) { if (id3 == ID_BLOCK) block(d3, s3); return true; });
            else if (id2 == ID_CLUSTER) walk_cluster(d2, s2);
            return true;
        });
    };
    bool ok = for_children(f, seg, seg_end, [&](uint32_t id1, uint64_t d1, uint64_t s1) {
        if (id1 == ID_INFO) {
            for_children(f, d1, d1 + s1, [&](uint32_t id2, uint64_t d2, uint64_t s2) {
                if (id2 == ID_TIMECODESCALE) timecode_scale = read_uint(f, d2, s2);
                if (id2 == ID_DURATION) duration = read_float(f, d2, s2);
                return true;
            });
        } else if (id1 == ID_TRACKS) {
            for_children(f, d1, d1 + s1, [&](uint32_t id2, uint64_t d2, uint64_t s2) {
                if (id2 != ID_TRACKENTRY || track >= 0) return true;
                int num = -1, type = 0, w = 0, hgt = 0;
                uint64_t dd = 0;
                std::string cid;
                std::vector<uint8_t> pv;
                for_children(f, d2, d2 + s2, [&](uint32_t id3, uint64_t d3, uint64_t s3) {
                    if (id3 == ID_TRACKNUMBER) num = (int)read_uint(f, d3, s3);
                    else if (id3 == ID_TRACKTYPE) type = (int)read_uint(f, d3, s3);
                    else if (id3 == ID_DEFAULTDURATION) dd = read_uint(f, d3, s3);
                    else if (id3 == ID_CODECID) { cid.resize((size_t)s3); f.read_at(d3, &cid[0], (size_t)s3); while (!cid.empty() && !cid.back()) cid.pop_back(); }
                    else if (id3 == ID_CODECPRIVATE) { pv.resize((size_t)s3); f.read_at(d3, pv.data(), (size_t)s3); }
                    else if (id3 == ID_VIDEO)
                        for_children(f, d3, d3 + s3, [&](uint32_t id4, uint64_t d4, uint64_t s4) {
                            if (id4 == ID_PIXELWIDTH) w = (int)read_uint(f, d4, s4);
                            if (id4 == ID_PIXELHEIGHT) hgt = (int)read_uint(f, d4, s4);
                            return true;
                        });
                    return true;
                });
                if (type == 1) { track = num; codec = cid; priv = pv; pw = w; ph = hgt; default_duration = dd; }
                return true;
            });
        } else if (id1 == ID_CLUSTER) walk_cluster(d1, s1);
        return true;
    });
    if (!ok && r.frames.empty()) return fail(ERR_FORMAT, "Matroska: damaged element structure");
    if (track < 0) return fail(ERR_FORMAT, "Matroska: no video track");
    const uint8_t* rec = nullptr;
    size_t rec_size = 0;
    if (codec == "V_FFV1") { rec = priv.data(); rec_size = priv.size(); }
    else if (codec == "V_MS/VFW/FOURCC") {
        if (priv.size() < 40 || memcmp(priv.data() + 16, "FFV1", 4) != 0)
            return fail(ERR_UNSUPPORTED, "Matroska video track is not FFV1 (VFW fourcc '%.4s')", priv.size() >= 20 ? (const char*)priv.data() + 16 : "?");
        rec = priv.data() + 40; rec_size = priv.size() - 40;
    } else return fail(ERR_UNSUPPORTED, "Matroska video track codec '%s': only FFV1 is decoded (H.264 and the like need a real FFmpeg)", codec.c_str());
    r.dec.W = pw; r.dec.H = ph;
    if (pw <= 0 || ph <= 0) return fail(ERR_FORMAT, "Matroska: no PixelWidth / PixelHeight");
    if (rec_size) {
        r.config.assign(rec, rec + rec_size);
        int rc = parse_config_record(rec, rec_size, r.dec.f);
        if (rc) return rc;
        r.dec.have_config = true;
        rc = r.dec.check_supported();
        if (rc) return rc;
    }
    std::stable_sort(r.frames.begin(), r.frames.end(), [](const FrameRef& a, const FrameRef& b) { return a.timecode < b.timecode; });
    mdvt_video_info& in = r.info;
    in.width = pw; in.height = ph; in.frames = (int64_t)r.frames.size();
    if (default_duration) in.fps = 1e9 / (double)default_duration;
    else if (duration > 0 && !r.frames.empty()) in.fps = (double)r.frames.size() / (duration * (double)timecode_scale * 1e-9);
    else if (r.frames.size() > 1) in.fps = (double)(r.frames.size() - 1) / ((double)(r.frames.back().timecode - r.frames.front().timecode) * (double)timecode_scale * 1e-9);
    return 0;
}

void fill_codec_info(mdvt_video_reader& r)
{
    const Ffv1Config& f = r.dec.f;
    r.info.ffv1_version = f.version; r.info.ffv1_micro_version = f.micro; r.info.coder_type = f.coder;
    r.info.slices = f.version >= 3 ? f.nh * f.nv : 1; r.info.alpha = f.alpha; r.info.intra = f.intra; r.info.ec = f.ec;
    r.info.pix_fmt = f.pix_fmt();
}

// ---- writer ----
struct EbmlBuf {
    std::vector<uint8_t> b;
    void id(uint32_t v) { if (v > 0xFFFFFF) b.push_back((uint8_t)(v >> 24)); if (v > 0xFFFF) b.push_back((uint8_t)(v >> 16)); if (v > 0xFF) b.push_back((uint8_t)(v >> 8)); b.push_back((uint8_t)v); }
    void size(uint64_t s)                   // shortest form
    {
        int n = 1;
        while (n < 8 && s >= (1ull << (7 * n)) - 1) ++n;
        size_n(s, n);
    }
    void size_n(uint64_t s, int n) { for (int i = n - 1; i >= 0; --i) b.push_back((uint8_t)((s >> (8 * i)) | (i == n - 1 ? (0x80u >> (n - 1)) : 0u))); }
    void uint_el(uint32_t i, uint64_t v) { int n = 1; while (n < 8 && (v >> (8 * n))) ++n; id(i); size((uint64_t)n); for (int k = n - 1; k >= 0; --k) b.push_back((uint8_t)(v >> (8 * k))); }
    void str_el(uint32_t i, const char* s) { id(i); size(strlen(s)); b.insert(b.end(), s, s + strlen(s)); }
    void bin_el(uint32_t i, const uint8_t* p, size_t n) { id(i); size(n); b.insert(b.end(), p, p + n); }
    void f64_el(uint32_t i, double v) { id(i); size(8); uint64_t u; memcpy(&u, &v, 8); for (int k = 7; k >= 0; --k) b.push_back((uint8_t)(u >> (8 * k))); }
    void master(uint32_t i, const EbmlBuf& c) { id(i); size(c.b.size()); b.insert(b.end(), c.b.begin(), c.b.end()); }
};

}  // namespace

struct mdvt_video_writer {
    FILE* fp = nullptr;
    int W = 0, H = 0, nh = 4, nv = 4;
    int fps_num = 30, fps_den = 1;
    int64_t frames = 0;
    uint64_t segment_data = 0;       // file offset of the Segment's first child
    uint64_t duration_pos = 0;       // file offset of the Duration's 8 data bytes
    uint64_t segment_size_pos = 0;   // file offset of the Segment's 8-byte size field
    std::vector<std::pair<uint64_t, uint64_t>> cues;     // timecode (ms), cluster position relative to segment_data
    std::vector<uint8_t> packet;
    int coder = 1, gop = 1;          // the stream class of mdvt_video_create_stream: coder 0, a key frame every gop frames
    std::vector<GolombSliceState> golomb;
    uint64_t frame_ms(int64_t k) const { return (uint64_t)((k * 1000 * (int64_t)fps_den + fps_num / 2) / fps_num); }
};

struct mdvt_ffv1_stream_decoder { Decoder dec; };

extern "C" {

const char* mdvt_video_last_error(void) { return g_err.c_str(); }
int mdvt_video_abi(void) { return MDVT_VIDEO_ABI; }

int mdvt_video_open(const char* path, mdvt_video_reader** out, mdvt_video_info* info)
{
    if (!path || !out) return fail(ERR_ARG, "NULL argument");
    *out = nullptr;
    mdvt_video_reader* r = new mdvt_video_reader();
    if (!r->file.open(path)) { delete r; return fail(ERR_IO, "cannot open %s", path); }
    int rc = index_matroska(*r);
    if (rc) { delete r; return rc; }
    if (r->frames.empty()) { delete r; return fail(ERR_FORMAT, "%s holds no video frames", path); }
    if (!r->dec.have_config) {
        // versions 0 / 1: the parameters are inside the first key frame -- decode it once into a scratch picture to learn them
        std::vector<uint8_t> scratch((size_t)r->info.width * 3 * (size_t)r->info.height);
        rc = mdvt_video_read(r, scratch.data(), (size_t)r->info.width * 3, MDVT_VIDEO_RGB, 0);
        if (rc < 0) { delete r; return rc; }
        r->next = 0;
        r->dec.key_frame_ok = false;
    }
    fill_codec_info(*r);
    if (info) *info = r->info;
    *out = r;
    return 0;
}

int mdvt_video_read(mdvt_video_reader* r, uint8_t* dst, size_t pitch, int order, int threads)
{
    if (!r || !dst) return fail(ERR_ARG, "NULL argument");
    if (pitch < (size_t)r->info.width * 3) return fail(ERR_ARG, "pitch smaller than one row");
    if (order != MDVT_VIDEO_RGB && order != MDVT_VIDEO_BGR) return fail(ERR_ARG, "order must be MDVT_VIDEO_RGB or MDVT_VIDEO_BGR");
    if (r->next >= r->frames.size()) return 1;
    const FrameRef& fr = r->frames[r->next];
    r->packet.resize(fr.size);
    if (!r->file.read_at(fr.offset, r->packet.data(), fr.size)) return fail(ERR_IO, "short read of frame %zu", r->next);
    const int rc = r->dec.decode_frame(r->packet.data(), r->packet.size(), dst, pitch, order, threads);
    if (rc) return rc;
    ++r->next;
    return 0;
}

int mdvt_video_rewind(mdvt_video_reader* r)
{
    if (!r) return fail(ERR_ARG, "NULL argument");
    r->next = 0;
    r->dec.key_frame_ok = false;
    return 0;
}

static int packet_is_key(mdvt_video_reader* r, size_t k)
{
    uint8_t b[2];
    if (r->frames[k].size < 2 || !r->file.read_at(r->frames[k].offset, b, 2)) return -1;
    RacDec c;
    c.init(b, 2);
    uint8_t st = 128;
    return c.get(&st);
}

int mdvt_video_seek(mdvt_video_reader* r, int64_t frame, int threads)
{
    if (!r) return fail(ERR_ARG, "NULL argument");
    if (frame < 0 || frame > (int64_t)r->frames.size()) return fail(ERR_ARG, "frame %lld outside 0..%zu", (long long)frame, r->frames.size());
    if ((size_t)frame == r->next && r->dec.key_frame_ok) return 0;
    if ((size_t)frame == r->frames.size()) { r->next = r->frames.size(); return 0; }
    size_t k = (size_t)frame;
    for (;; --k) {
        const int key = packet_is_key(r, k);
        if (key < 0) return fail(ERR_IO, "short read of frame %zu", k);
        if (key) break;
        if (k == 0) return fail(ERR_DATA, "no key frame at or before frame %lld", (long long)frame);
    }
    r->dec.key_frame_ok = false;
    r->next = k;
    if (k == (size_t)frame) return 0;
    std::vector<uint8_t> scratch((size_t)r->info.width * 3 * (size_t)r->info.height);
    while (r->next < (size_t)frame) {
        const int rc = mdvt_video_read(r, scratch.data(), (size_t)r->info.width * 3, MDVT_VIDEO_RGB, threads);
        if (rc) return rc < 0 ? rc : fail(ERR_DATA, "unexpected end of the video");
    }
    return 0;
}

int mdvt_video_next_packet(mdvt_video_reader* r, uint8_t* packet, size_t packet_cap, size_t* packet_size)
{
    if (!r || !packet || !packet_size) return fail(ERR_ARG, "NULL argument");
    if (r->next >= r->frames.size()) return 1;
    const FrameRef& fr = r->frames[r->next];
    if (fr.size > packet_cap) return fail(ERR_ARG, "packet buffer too small: %u needed", fr.size);
    if (!r->file.read_at(fr.offset, packet, fr.size)) return fail(ERR_IO, "short read of frame %zu", r->next);
    *packet_size = fr.size;
    ++r->next;
    r->dec.key_frame_ok = false;          // the decoder did not see this frame: the next decode must start at a key frame
    return 0;
}

int mdvt_video_config_record(mdvt_video_reader* r, uint8_t* config, size_t config_cap, size_t* config_size)
{
    if (!r || !config_size) return fail(ERR_ARG, "NULL argument");
    if (r->config.size() > config_cap || (!config && !r->config.empty())) return fail(ERR_ARG, "config buffer too small: %zu needed", r->config.size());
    if (!r->config.empty()) memcpy(config, r->config.data(), r->config.size());
    *config_size = r->config.size();
    return 0;
}

void mdvt_video_close(mdvt_video_reader* r) { delete r; }

int mdvt_ffv1_encode_frame(int width, int height, int slices_h, int slices_v, const uint8_t* src, size_t pitch, int order, int threads,
                           uint8_t* packet, size_t packet_cap, size_t* packet_size, uint8_t* config, size_t config_cap, size_t* config_size)
{
    if (!src || !packet || !packet_size || width < 1 || height < 1 || slices_h < 1 || slices_v < 1 || slices_h > width || slices_v > height)
        return fail(ERR_ARG, "bad argument");
    std::vector<uint8_t> pkt;
    int rc = encode_frame(width, height, slices_h, slices_v, src, pitch, order, threads, pkt);
    if (rc) return rc;
    if (pkt.size() > packet_cap) return fail(ERR_ARG, "packet buffer too small: %zu needed", pkt.size());
    memcpy(packet, pkt.data(), pkt.size());
    *packet_size = pkt.size();
    if (config && config_size) {
        const std::vector<uint8_t> rec = make_config_record(slices_h, slices_v);
        if (rec.size() > config_cap) return fail(ERR_ARG, "config buffer too small");
        memcpy(config, rec.data(), rec.size());
        *config_size = rec.size();
    }
    return 0;
}

int mdvt_ffv1_decode_frame(int width, int height, const uint8_t* config, size_t config_size, const uint8_t* packet, size_t packet_size,
                           uint8_t* dst, size_t pitch, int order, int threads)
{
    if (!config || !packet || !dst || width < 1 || height < 1 || pitch < (size_t)width * 3) return fail(ERR_ARG, "bad argument");
    Decoder dec;
    dec.W = width; dec.H = height;
    int rc = parse_config_record(config, config_size, dec.f);
    if (rc) return rc;
    dec.have_config = true;
    rc = dec.check_supported();
    if (rc) return rc;
    return dec.decode_frame(packet, packet_size, dst, pitch, order, threads);
}

static int create_writer(const char* path, int width, int height, int fps_num, int fps_den, int slices_h, int slices_v, int coder, int gop,
                         mdvt_video_writer** out)
{
    if (!path || !out || width < 1 || height < 1 || fps_num < 1 || fps_den < 1) return fail(ERR_ARG, "bad argument");
    if (slices_h == 0 && slices_v == 0) { slices_h = std::min(4, width); slices_v = std::min(4, height); }
    if (slices_h < 1 || slices_v < 1 || slices_h > width || slices_v > height || slices_h * slices_v > 1024) return fail(ERR_ARG, "bad slice counts");
    *out = nullptr;
    mdvt_video_writer* w = new mdvt_video_writer();
    w->fp = fopen(path, "wb");
    if (!w->fp) { delete w; return fail(ERR_IO, "cannot create %s", path); }
    w->W = width; w->H = height; w->nh = slices_h; w->nv = slices_v; w->fps_num = fps_num; w->fps_den = fps_den;
    w->coder = coder; w->gop = gop;
    EbmlBuf head, eb;
    eb.uint_el(ID_EBMLVERSION, 1); eb.uint_el(ID_EBMLREADVERSION, 1); eb.uint_el(ID_EBMLMAXIDLENGTH, 4); eb.uint_el(ID_EBMLMAXSIZELENGTH, 8);
    eb.str_el(ID_DOCTYPE, "matroska"); eb.uint_el(ID_DOCTYPEVERSION, 4); eb.uint_el(ID_DOCTYPEREADVERSION, 2);
    head.master(ID_EBML, eb);
    head.id(ID_SEGMENT);
    w->segment_size_pos = head.b.size();
    head.size_n(0, 8);                                   // patched by mdvt_video_finish
    w->segment_data = head.b.size();
    EbmlBuf info;
    info.uint_el(ID_TIMECODESCALE, 1000000);
    info.str_el(ID_MUXINGAPP, "mdvt_video");
    info.str_el(ID_WRITINGAPP, "metric_depth_video_toolbox_amd");
    info.id(ID_DURATION); info.size(8);
    const size_t dur_in_info = info.b.size();
    for (int k = 0; k < 8; ++k) info.b.push_back(0);
    head.id(ID_INFO); head.size(info.b.size());
    w->duration_pos = head.b.size() + dur_in_info;
    head.b.insert(head.b.end(), info.b.begin(), info.b.end());
    EbmlBuf video, entry, tracks;
    video.uint_el(ID_PIXELWIDTH, (uint64_t)width); video.uint_el(ID_PIXELHEIGHT, (uint64_t)height);
    entry.uint_el(ID_TRACKNUMBER, 1); entry.uint_el(ID_TRACKUID, 1); entry.uint_el(ID_TRACKTYPE, 1); entry.uint_el(ID_FLAGLACING, 0);
    entry.uint_el(ID_DEFAULTDURATION, (uint64_t)((1000000000.0 * fps_den) / fps_num + 0.5));
    entry.str_el(ID_CODECID, "V_FFV1");
    const std::vector<uint8_t> rec = make_config_record(slices_h, slices_v, coder, coder ? 1 : 0);
    entry.bin_el(ID_CODECPRIVATE, rec.data(), rec.size());
    entry.master(ID_VIDEO, video);
    tracks.master(ID_TRACKENTRY, entry);
    head.master(ID_TRACKS, tracks);
    if (fwrite(head.b.data(), 1, head.b.size(), w->fp) != head.b.size()) { fclose(w->fp); delete w; return fail(ERR_IO, "write failed"); }
    *out = w;
    return 0;
}

int mdvt_video_create(const char* path, int width, int height, int fps_num, int fps_den, int slices_h, int slices_v, mdvt_video_writer** out)
{
    return create_writer(path, width, height, fps_num, fps_den, slices_h, slices_v, 1, 1, out);
}

int mdvt_video_create_stream(const char* path, int width, int height, int fps_num, int fps_den, int slices_h, int slices_v, int coder_type,
                             int gop, mdvt_video_writer** out)
{
    if (coder_type != 0) return fail(ERR_ARG, "coder_type %d: the stream class is Golomb-Rice (0); mdvt_video_create writes the range coder's", coder_type);
    if (gop < 1) return fail(ERR_ARG, "gop must be >= 1");
    return create_writer(path, width, height, fps_num, fps_den, slices_h, slices_v, 0, gop, out);
}

int mdvt_video_write(mdvt_video_writer* w, const uint8_t* src, size_t pitch, int order, int threads)
{
    if (!w || !src) return fail(ERR_ARG, "NULL argument");
    if (pitch < (size_t)w->W * 3) return fail(ERR_ARG, "pitch smaller than one row");
    if (order != MDVT_VIDEO_RGB && order != MDVT_VIDEO_BGR) return fail(ERR_ARG, "order must be MDVT_VIDEO_RGB or MDVT_VIDEO_BGR");
    int rc = w->coder ? encode_frame(w->W, w->H, w->nh, w->nv, src, pitch, order, threads, w->packet)
                      : encode_frame_golomb(w->W, w->H, w->nh, w->nv, src, pitch, order, threads, w->frames % w->gop == 0, w->golomb, w->packet);
    if (rc) return rc;
    return mdvt_video_write_packet(w, w->packet.data(), w->packet.size());
}

int mdvt_video_write_packet(mdvt_video_writer* w, const uint8_t* packet, size_t packet_size)
{
    if (!w || !packet || packet_size < 8) return fail(ERR_ARG, "bad argument");
    // one Cluster per frame; a key frame (every frame of the default, intra-only class) is flagged in its block and gets a cue: a seek
    // point.  An inter frame of the stream class is neither.
    const uint64_t tc = w->frame_ms(w->frames);
    EbmlBuf cl, body;
    body.uint_el(ID_TIMECODE, tc);
    body.id(ID_SIMPLEBLOCK); body.size(packet_size + 4);
    RacDec kc;
    uint8_t kst = 128;
    const bool key = kc.init(packet, 2) && kc.get(&kst);                                            // the packet's first range-coded bit
    body.b.push_back(0x81); body.b.push_back(0); body.b.push_back(0); body.b.push_back(key ? 0x80 : 0x00);   // track 1, relative time 0, key frame
    cl.id(ID_CLUSTER); cl.size(body.b.size() + packet_size);
    const uint64_t pos = (uint64_t)ftello(w->fp);
    if (fwrite(cl.b.data(), 1, cl.b.size(), w->fp) != cl.b.size() || fwrite(body.b.data(), 1, body.b.size(), w->fp) != body.b.size() ||
        fwrite(packet, 1, packet_size, w->fp) != packet_size)
        return fail(ERR_IO, "write failed (disk full?)");
    if (key) w->cues.push_back({tc, pos - w->segment_data});
    ++w->frames;
    return 0;
}

int mdvt_video_seek_packet(mdvt_video_reader* r, int64_t frame)
{
    if (!r) return fail(ERR_ARG, "NULL argument");
    if (frame < 0 || frame > (int64_t)r->frames.size()) return fail(ERR_ARG, "frame %lld outside 0..%zu", (long long)frame, r->frames.size());
    r->next = (size_t)frame;
    r->dec.key_frame_ok = false;          // nothing is decoded on the way: the next decode must start at a key frame
    return 0;
}

int mdvt_video_packet_is_key(mdvt_video_reader* r, int64_t frame)
{
    if (!r) return fail(ERR_ARG, "NULL argument");
    if (frame < 0 || frame >= (int64_t)r->frames.size()) return fail(ERR_ARG, "frame %lld outside 0..%zu", (long long)frame, r->frames.size());
    const int key = packet_is_key(r, (size_t)frame);
    return key < 0 ? fail(ERR_IO, "short read of frame %lld", (long long)frame) : key;
}

int mdvt_ffv1_stream_decoder_create(int width, int height, const uint8_t* config, size_t config_size, mdvt_ffv1_stream_decoder** out)
{
    if (!config || !out || width < 1 || height < 1) return fail(ERR_ARG, "bad argument");
    *out = nullptr;
    mdvt_ffv1_stream_decoder* d = new mdvt_ffv1_stream_decoder();
    d->dec.W = width; d->dec.H = height;
    int rc = parse_config_record(config, config_size, d->dec.f);
    if (!rc) { d->dec.have_config = true; rc = d->dec.check_supported(); }
    if (rc) { delete d; return rc; }
    *out = d;
    return 0;
}

int mdvt_ffv1_stream_decoder_decode(mdvt_ffv1_stream_decoder* d, const uint8_t* packet, size_t packet_size, uint8_t* dst, size_t pitch, int order,
                                    int threads)
{
    if (!d || !packet || !dst || pitch < (size_t)d->dec.W * 3) return fail(ERR_ARG, "bad argument");
    if (order != MDVT_VIDEO_RGB && order != MDVT_VIDEO_BGR) return fail(ERR_ARG, "order must be MDVT_VIDEO_RGB or MDVT_VIDEO_BGR");
    return d->dec.decode_frame(packet, packet_size, dst, pitch, order, threads);
}

void mdvt_ffv1_stream_decoder_destroy(mdvt_ffv1_stream_decoder* d) { delete d; }

int mdvt_video_finish(mdvt_video_writer* w, int64_t* frames)
{
    if (!w) return fail(ERR_ARG, "NULL argument");
    int rc = 0;
    EbmlBuf cues;
    for (auto& c : w->cues) {
        EbmlBuf pos, pt;
        pos.uint_el(ID_CUETRACK, 1); pos.uint_el(ID_CUECLUSTERPOSITION, c.second);
        pt.uint_el(ID_CUETIME, c.first); pt.master(ID_CUETRACKPOSITIONS, pos);
        cues.master(ID_CUEPOINT, pt);
    }
    EbmlBuf tail;
    tail.master(ID_CUES, cues);
    if (fwrite(tail.b.data(), 1, tail.b.size(), w->fp) != tail.b.size()) rc = fail(ERR_IO, "write failed");
    const uint64_t end = (uint64_t)ftello(w->fp);
    EbmlBuf sz;
    sz.size_n(end - w->segment_data, 8);
    uint8_t dur[8];
    const double d = (double)w->frame_ms(w->frames);
    uint64_t u;
    memcpy(&u, &d, 8);
    for (int k = 0; k < 8; ++k) dur[k] = (uint8_t)(u >> (8 * (7 - k)));
    if (fseeko(w->fp, (off_t)w->segment_size_pos, SEEK_SET) || fwrite(sz.b.data(), 1, 8, w->fp) != 8 ||
        fseeko(w->fp, (off_t)w->duration_pos, SEEK_SET) || fwrite(dur, 1, 8, w->fp) != 8)
        rc = fail(ERR_IO, "patching the headers failed");
    if (fclose(w->fp)) rc = fail(ERR_IO, "close failed");
    if (frames) *frames = w->frames;
    delete w;
    return rc;
}

}  // extern "C"
