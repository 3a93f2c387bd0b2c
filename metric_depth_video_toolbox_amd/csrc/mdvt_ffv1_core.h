// mdvt_ffv1_core.h -- the project's one definition of the FFV1 (RFC 9043) primitives: the tables, the CRC, the range decoder and
// its integer binarisation, the bit reader, the Golomb-Rice symbol reader with its context state, the run-length exponents, the
// predictor, the pixel stores, the slice-table walk and the key-frame bit.  The host codec (csrc_host/, libmdvt_video.so), the device
// encoder (mdvt_ffv1.hip), the two device decode kernels (mdvt_ffv1_decode.hip, mdvt_ffv1_stream_decode.hip), the C ABI
// (mdvt_api.hip) and the host test programs are all built on it.  Plain C++: it compiles for the host alone (g++, where the tests
// run it under the sanitizers) and for host + device under hipcc; no HIP intrinsic, no recursion, and no allocation.  What is
// marked (host) is not compiled for the device.
//
// On top of the primitives it holds the device's decoder: SliceDec and parse_stream_class, for version 3, RGB (JPEG 2000 RCT) or
// YCbCr, 8 bits, no alpha, the default 666-context quantisation tables.  The host's decoder (csrc_host/mdvt_ffv1_dec.cpp) is the
// general one -- any quantisation tables, initial states, alpha, versions 0 and 1 -- over the same primitives, and every GPU decode
// test holds SliceDec to its bytes.  The two entry points ask the record parser and SliceDec for different classes of the format:
//   intra    (mdvt_decode_video_frames)   the range coder with the default state table, key frames only: every slice of every
//                                         frame starts from fresh context state
//   stream   (mdvt_decode_video_stream)   Golomb-Rice or the range coder, key and inter frames: the context state carries from
//                                         frame to frame of a key-frame run, and the caller resets it at a key frame.  This class
//                                         also holds YCbCr (colorspace_type 0; 4:4:4, 4:2:2, 4:2:0): SliceDec's planar mode, in
//                                         which a slice is plane Y row by row, then Cb, then Cr, 8-bit samples, and the store side
//                                         converts to RGB (store_ycbcr_pixel) once a row of Cr is there
// Nothing read from a packet steers a loop or an address: every loop runs to a count fixed by the frame's geometry, bytes and bits
// past a slice's end read as zero (the host's overread, which the range coder counts), a symbol's exponent loop has the RFC's
// bound, a context index is bounded by the quantisation arithmetic (|ctx| <= 665), a run length is consumed sample by sample
// inside the row's loop, and run_index is held inside log2_run's domain whatever the bits say.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MDVT_HD __host__ __device__ inline
#else
#define MDVT_HD inline
#endif

namespace mdvt_ffv1 {

constexpr int kContexts = (11 * 11 * 11 + 1) / 2;         // 666
constexpr int kStateBytes = kContexts * 32;                // one state set
constexpr int kMaxSlices = 1024;                           // slices per frame the device codes / decodes

// per-frame status words (include/mdvt_ffv1_decode.h); the largest of a frame's slices wins.  The last two are
// mdvt_decode_video_stream's alone (include/mdvt_ffv1_stream_decode.h)
enum : uint32_t { kOk = 0, kCrcMismatch = 1, kBadSliceHeader = 2, kDamaged = 3, kBadPacket = 4, kNoKeyFrame = 5, kBrokenRun = 6 };

// FFmpeg's quant11 (ffv1enc.c): the 11-level quantisation of (difference & 0xFF), with the i == 128 entry at -5
MDVT_HD int quant11(int i)
{
    const int d = i < 128 ? i : i - 256;
    const int a = d < 0 ? -d : d;
    int q = a == 0 ? 0 : a < 2 ? 1 : a < 5 ? 2 : a < 12 ? 3 : a < 32 ? 4 : 5;
    if (i == 128) q = 5;
    return d < 0 ? -q : q;
}

MDVT_HD int median3(int a, int b, int c)
{
    return a > b ? (b > c ? b : (a > c ? c : a)) : (a > c ? a : (b > c ? c : b));
}

// the default state-transition table (RFC 9043 section 3.8.1.3), generated the way FFmpeg's ff_build_rac_states(0.05 * 2^32, 256 - 8)
// generates it; tests/test_ffv1_cpu.py checks it against the RFC's table
inline void default_states(uint8_t* zero, uint8_t* one_state)
{
    const long long one = 1LL << 32;
    const int factor = (int)(0.05 * (double)(1LL << 32));
    const int max_p = 256 - 8;
    for (int k = 0; k < 256; ++k) { zero[k] = 0; one_state[k] = 0; }
    int last_p8 = 0;
    long long p = one / 2;
    for (int k = 0; k < 128; ++k) {
        int p8 = (int)((256 * p + one / 2) >> 32);
        if (p8 <= last_p8) p8 = last_p8 + 1;
        if (last_p8 && last_p8 < 256 && p8 <= max_p) one_state[last_p8] = (uint8_t)p8;
        p += ((one - p) * factor + one / 2) >> 32;
        last_p8 = p8;
    }
    for (int k = 256 - max_p; k <= max_p; ++k) {
        if (one_state[k]) continue;
        p = (k * one + 128) >> 8;
        p += ((one - p) * factor + one / 2) >> 32;
        int p8 = (int)((256 * p + one / 2) >> 32);
        if (p8 <= k) p8 = k + 1;
        if (p8 > max_p) p8 = max_p;
        one_state[k] = (uint8_t)p8;
    }
    for (int k = 1; k < 255; ++k) zero[k] = (uint8_t)(256 - one_state[256 - k]);
}

// (host) RacDec's table, next[s] = zero_state[s] | one_state[s] << 8, of the default states
inline const uint16_t* default_next_states()
{
    static const struct Table {
        uint16_t next[256];
        Table()
        {
            uint8_t zero[256], one[256];
            default_states(zero, one);
            for (int k = 0; k < 256; ++k) next[k] = (uint16_t)(zero[k] | (one[k] << 8));
        }
    } table;
    return table.next;
}

// (host) ... and of a stream's own one_state[1 .. 255] (coder_type 2): zero_state[s] = 256 - one_state[256 - s]
inline void custom_next_states(const uint8_t* one_state, uint16_t* next)
{
    next[0] = (uint16_t)(one_state[0] << 8);
    for (int k = 1; k < 256; ++k) next[k] = (uint16_t)((uint8_t)(256 - one_state[256 - k]) | (one_state[k] << 8));
}

// ---- CRC-32, generator 0x04C11DB7, most significant bit first, initial value 0, no final XOR ----
MDVT_HD uint32_t crc_table_entry(uint32_t k)
{
    uint32_t v = k << 24;
    for (int b = 0; b < 8; ++b) v = (v << 1) ^ ((v & 0x80000000u) ? 0x04C11DB7u : 0u);
    return v;
}

// (host) the CRC of n more bytes, through the table of crc_table_entry
inline uint32_t crc32_msb(uint32_t crc, const uint8_t* p, size_t n)
{
    static const struct Table {
        uint32_t t[256];
        Table() { for (uint32_t k = 0; k < 256; ++k) t[k] = crc_table_entry(k); }
    } table;
    for (size_t i = 0; i < n; ++i) crc = (crc << 8) ^ table.t[(crc >> 24) ^ p[i]];
    return crc;
}

// a(x) * b(x) mod P(x), P = 0x104C11DB7, most significant bit = highest power
MDVT_HD uint32_t gf2_mulmod(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int k = 31; k >= 0; --k) {
        r = (r << 1) ^ ((r & 0x80000000u) ? 0x04C11DB7u : 0u);
        if ((b >> k) & 1u) r ^= a;
    }
    return r;
}

// crc * x^(8 n) mod P: the CRC of a chunk followed by n more bytes (initial value 0, no final XOR: the CRC is linear)
MDVT_HD uint32_t crc_shift(uint32_t crc, uint32_t n)
{
    uint32_t p = 0x100u;                                   // x^8
    for (; n && crc; n >>= 1) {                            // (at most 32 rounds)
        if (n & 1u) crc = gf2_mulmod(crc, p);
        p = gf2_mulmod(p, p);
    }
    return crc;
}

// ---- the slice table: every slice ends in a 24-bit payload size (+ an error byte + a CRC-32 when ec), so the extents are found
// by walking back from the packet's end (the host reader's checks, Decoder::decode_frame).  `byte(k)` reads packet byte k < size.
// n <= kMaxSlices steps.  -> kOk, or kBadPacket with nothing in off / len to be used. ----
template <class Byte>
MDVT_HD uint32_t walk_slices(Byte byte, uint32_t size, int n, int ec, uint32_t* off, uint32_t* len)
{
    if (size < 3u) return kBadPacket;
    const uint32_t trailer = 3u + (ec ? 5u : 0u);
    uint32_t end = size;
    for (int i = n - 1; i >= 0; --i) {
        if (end < trailer) return kBadPacket;                                    // "packet too short for n slices"
        const uint32_t t = end - trailer;
        const uint32_t payload = ((uint32_t)byte(t) << 16) | ((uint32_t)byte(t + 1u) << 8) | (uint32_t)byte(t + 2u);
        if (payload + trailer > end) return kBadPacket;                          // "slice i claims ... bytes"
        off[i] = end - trailer - payload;
        len[i] = payload;
        end = off[i];
    }
    return end ? kBadPacket : kOk;                                               // "stray bytes before the first slice"
}

// ---- the range decoder over a byte source: Src::byte(k) for k < avail ----
template <class Src>
struct RacDec {
    Src src;
    uint32_t pos, end;             // next byte, and the first byte that reads as zero
    int low, range, overread;
    const uint16_t* next;          // next[s] = zero_state[s] | one_state[s] << 8: one lookup per decision, whatever the bit

    // (host) starts the coder on the `size` bytes of s: false when there are fewer than two.  (SliceDec::begin does the same by hand,
    // as the first slice's coder starts on the whole packet)
    bool init(Src s, uint32_t size, const uint16_t* next_)
    {
        if (size < 2u) return false;
        src = s; next = next_; pos = 2; end = size; range = 0xFF00; overread = 0;
        low = ((int)s.byte(0) << 8) | (int)s.byte(1);
        if (low >= 0xFF00) { low = 0xFF00; end = 2; }
        return true;
    }

    MDVT_HD int get(uint8_t* state)
    {
        const int s = *state;
        const unsigned t = next[s];
        const int range1 = (range * s) >> 8;
        range -= range1;
        int bit;
        if (low < range) { *state = (uint8_t)t; bit = 0; }
        else { low -= range; range = range1; *state = (uint8_t)(t >> 8); bit = 1; }
        if (range < 0x100) {
            range <<= 8; low <<= 8;
            if (pos < end) low += src.byte(pos++);
            else ++overread;
        }
        return bit;
    }

    // the range-coded integer binarisation (RFC 9043 section 3.8.1.2): 32 states per context; the exponent has the RFC's bound
    MDVT_HD int symbol(uint8_t* state, bool is_signed, bool* bad)
    {
        if (get(state)) return 0;
        int e = 0;
        while (get(state + 1 + (e < 9 ? e : 9))) {
            if (++e > 31) { *bad = true; return 0; }
        }
        unsigned a = 1;
        for (int i = e - 1; i >= 0; --i) a += a + (unsigned)get(state + 22 + (i < 9 ? i : 9));
        const int neg = (is_signed && get(state + 11 + (e < 10 ? e : 10))) ? -1 : 0;
        return (int)((a ^ (unsigned)neg) - (unsigned)neg);
    }
};
// ---- Golomb-Rice (RFC 9043 section 3.8.2), and what the stream class needs besides ----
// the walk's word per frame: the packet's slice table holds and its key-frame bit is clear / set, or the packet is refused
enum : uint32_t { kFrameInter = 0, kFrameKey = 1, kFrameBad = 2 };

// the key-frame bit as RacDec decides it: the first decision of the packet's range coder, state 128 (b0, b1: the first two bytes)
MDVT_HD int key_frame_bit(uint8_t b0, uint8_t b1)
{
    int low = ((int)b0 << 8) | (int)b1;
    if (low >= 0xFF00) low = 0xFF00;
    return low >= 0xFF00 - ((0xFF00 * 128) >> 8);
}

MDVT_HD int clz32(uint32_t v) { return v ? __builtin_clz(v) : 32; }

// The bit reader over a byte source: bits [0, 8 * nbytes) of the bytes from `base` on, most significant bit first; every bit
// past them is zero.  A 64-bit accumulator holds the next `n` bits at its top, refilled a byte at a time through Src::byte (which
// keeps its own window of aligned words on the device).
template <class Src>
struct BitReader {
    Src src;
    uint32_t base, nbytes, next;   // next: the first byte (from base) not yet in the accumulator; it stops at nbytes
    uint64_t acc;
    int n;

    MDVT_HD void init(Src s, uint32_t base_, uint32_t nbytes_) { src = s; base = base_; nbytes = nbytes_; next = 0; acc = 0; n = 0; }
    MDVT_HD void refill()                                  // -> n > 56
    {
        while (n <= 56) {
            uint64_t b = 0;
            if (next < nbytes) { b = src.byte(base + next); ++next; }
            acc |= b << (56 - n);
            n += 8;
        }
    }
    MDVT_HD unsigned get(int k)                            // 0 <= k <= 32
    {
        if (k == 0) return 0u;
        if (n < k) refill();
        const unsigned v = (unsigned)(acc >> (64 - k));
        acc <<= k; n -= k;
        return v;
    }
    // zeros up to the next one bit, at most `limit` (<= 32) of them: consumes the zeros, and the one when there are fewer than `limit`
    MDVT_HD int zeros(int limit)
    {
        if (n < limit + 1) refill();
        int q = clz32((uint32_t)(acc >> 32));
        if (q >= limit) { acc <<= limit; n -= limit; return limit; }
        acc <<= q + 1; n -= q + 1;
        return q;
    }
};

// one context of the Golomb-Rice coder; vlc_reset gives its initial value
struct VlcState { int16_t drift; uint16_t error_sum; int8_t bias; uint8_t count; };
constexpr int kVlcBytes = kContexts * (int)sizeof(VlcState);       // one set: 666 x 6 bytes
MDVT_HD void vlc_reset(VlcState* v) { v->drift = 0; v->error_sum = 4; v->bias = 0; v->count = 1; }

constexpr int kRunIndexMax = 40;
// (a function, not a table at namespace scope: one definition for host and device)
MDVT_HD int log2_run(int run_index)
{
    return run_index < 16 ? run_index >> 2 : run_index < 24 ? 4 + ((run_index - 16) >> 1) : run_index - 16;
}

struct NoStats {
    MDVT_HD void escape() {}
    MDVT_HD void halving() {}
    MDVT_HD void run_index(int) {}
    MDVT_HD void short_tail_run() {}
};

// get_ur_golomb(k, limit 12, esc_len kBits) folded to a signed value: q zeros + a one + k bits -> (q << k) | bits; 12 zeros ->
// kBits bits + 11.  kBits: the bits of a sample, 9 for the RCT's planes, 8 for YCbCr's
template <int kBits, class Src, class Stats>
MDVT_HD int get_sr_golomb(BitReader<Src>& gb, int k, Stats& stats)
{
    const int q = gb.zeros(12);
    unsigned v;
    if (q < 12) v = ((unsigned)q << k) | gb.get(k);
    else { v = gb.get(kBits) + 11u; stats.escape(); }
    return (int)(v >> 1) ^ -(int)(v & 1u);
}

// one Golomb-Rice coded sample difference of kBits bits, with update_vlc_state
template <int kBits, class Src, class Stats>
MDVT_HD int get_vlc_symbol(BitReader<Src>& gb, VlcState* st, Stats& stats)
{
    int i = st->count, k = 0;
    while (i < st->error_sum) { ++k; i += i; }             // (count >= 1 and error_sum < 2^16: at most 16 rounds)
    int v = get_sr_golomb<kBits>(gb, k, stats);
    v ^= ((2 * st->drift + st->count) >> 31);
    const int ret = (((v + st->bias) + (1 << (kBits - 1))) & ((1 << kBits) - 1)) - (1 << (kBits - 1));      // fold(., kBits)
    int drift = st->drift, count = st->count;
    int es = st->error_sum + (v < 0 ? -v : v);
    drift += v;
    if (count == 128) { count >>= 1; drift >>= 1; es >>= 1; stats.halving(); }
    ++count;
    if (drift <= -count) {
        st->bias = (int8_t)(st->bias - 1 > -128 ? st->bias - 1 : -128);
        drift = drift + count > -count + 1 ? drift + count : -count + 1;
    } else if (drift > 0) {
        st->bias = (int8_t)(st->bias + 1 < 127 ? st->bias + 1 : 127);
        drift = drift - count < 0 ? drift - count : 0;
    }
    st->drift = (int16_t)drift; st->count = (uint8_t)count; st->error_sum = (uint16_t)es;
    return ret;
}

// ---- one slice ----
// the bytes of two context-state sets (luma, chroma): range coder 2 x 666 x 32, Golomb-Rice VlcState[2][666]; both multiples of 4
MDVT_HD size_t state_bytes(int coder) { return 2u * (size_t)(coder ? kStateBytes : kVlcBytes); }

// The JPEG 2000 RCT undone for one pixel: the samples of SliceDec's three planes (Y, Cb + 256, Cr + 256) -> the bytes o[ri], o[gi], o[bi]
MDVT_HD void store_rct_pixel(int y, int cb, int cr, uint8_t* o, int ri, int gi, int bi)
{
    int g = y, b = cb - 256, r = cr - 256;
    g -= (b + r) >> 2;
    b += g; r += g;
    o[ri] = (uint8_t)r; o[gi] = (uint8_t)g; o[bi] = (uint8_t)b;
}

// YCbCr -> the bytes o[ri], o[gi], o[bi] as include/mdvt_video.h decrees it: BT.601 limited range in integers (a decree of this
// project's, not a claim about swscale's bits)
MDVT_HD uint8_t clip8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
MDVT_HD void store_ycbcr_pixel(int y, int u, int v, uint8_t* o, int ri, int gi, int bi)
{
    const int c = y - 16, d = u - 128, e = v - 128;
    o[ri] = clip8((298 * c + 409 * e + 128) >> 8);
    o[gi] = clip8((298 * c - 100 * d - 208 * e + 128) >> 8);
    o[bi] = clip8((298 * c + 516 * d + 128) >> 8);
}

// The store side of SliceDec's planar mode, for `lanes` workers of which this is `lane`.  `l`: row y of plane p as plane_row() left
// it; `rect`: the slice's first pixel in the frame, rows `pitch` bytes apart; hs, vs: the log2 chroma subsampling; csw: the chroma
// rectangle's width.  The planes of a slice arrive one after another, so luma and Cb wait inside the slice's own pixels, which
// are all overwritten in the end: a row of Y goes to byte 0 of its pixels, a row of Cb to byte 1 of the top left pixel of each
// sample's 2^hs x 2^vs block, and a row of Cr converts the blocks of its samples -- one worker per block, which reads the block's Y
// and Cb before it writes the block's pixels.  Every address depends on the geometry alone.
MDVT_HD void planar_store_row(const int16_t* l, int p, int y, uint8_t* rect, size_t pitch, int sw, int sh, int csw, int hs, int vs, int ri,
                              int bi, int lane, int lanes)
{
    if (p == 0) {
        uint8_t* o = rect + (size_t)y * pitch;
        for (int x = lane; x < sw; x += lanes) o[3 * x] = (uint8_t)l[x];
        return;
    }
    const int ya = y << vs;
    uint8_t* top = rect + (size_t)ya * pitch;
    if (p == 1) {
        for (int cx = lane; cx < csw; cx += lanes) top[3 * (cx << hs) + 1] = (uint8_t)l[cx];
        return;
    }
    const int rows = sh - ya < (1 << vs) ? sh - ya : (1 << vs);
    for (int cx = lane; cx < csw; cx += lanes) {
        const int xa = cx << hs;
        const int cols = sw - xa < (1 << hs) ? sw - xa : (1 << hs);
        uint8_t* o = top + 3 * xa;
        const int u = o[1], v = l[cx];
        int yy[4] = {0, 0, 0, 0};
        for (int dy = 0; dy < rows; ++dy)
            for (int dx = 0; dx < cols; ++dx) yy[2 * dy + dx] = o[(size_t)dy * pitch + 3 * dx];
        for (int dy = 0; dy < rows; ++dy)
            for (int dx = 0; dx < cols; ++dx) store_ycbcr_pixel(yy[2 * dy + dx], u, v, o + (size_t)dy * pitch + 3 * dx, ri, 1, bi);
    }
}

// One slice of one frame (the host's Decoder::slices[index] with decode_slice).  kGolomb = false leaves the Golomb-Rice side out
// of the compiled code: the intra class, whose coder_type is 1 whatever begin() is told.  The caller owns the memory: `st` the
// context state (state_bytes(coder)), which it resets (reset_state(), or its own fill) where a run begins and leaves alone
// otherwise; `lines` three planes x three row slots x `stride` samples (stride >= slice width + 2), all zero before every frame;
// `misc` 64 bytes; q11[256] = quant11.  Per frame: begin() reads the key-frame bit (first slice: left in `key` for the caller to
// judge), the slice header and, for coder_type 0, the sentinel bit, and starts the bit reader where the host starts it; row(y)
// decodes the three planes of slice row y into slot y % 3 (sample k of plane p at lines[(p * 3 + y % 3) * stride + 1 + k]);
// finish() gives the status.  Planar mode (begin's `planar`: a YCbCr stream with log2 chroma subsampling hs, vs): the caller asks
// for plane_row(p, y) instead, in coding order -- plane 0 rows 0 .. sh - 1, then plane 1 and plane 2 rows 0 .. csh - 1 --, which
// decodes row y of plane p (8-bit samples, sw or csw of them) into plane p's slot y % 3.
template <class Src, bool kGolomb = false, class Stats = NoStats>
struct SliceDec {
    RacDec<Src> c;
    BitReader<Src> gb;
    uint8_t* st; int16_t* lines; uint8_t* misc; const int8_t* q11;
    int stride, sw, sh, x0, y0, cell;        // cell: the slice's index in the frame's nh x nv grid
    int csw, csh;                            // planar mode: the chroma rectangle, ceil(sw / 2^hs) x ceil(sh / 2^vs)
    int coder, run_index, key;               // key: the packet's key-frame bit, read by the frame's first slice (else 0)
    bool error;
    Stats stats;

    MDVT_HD bool golomb() const { return kGolomb && !coder; }
    MDVT_HD void reset_state()                             // (the kernels do this with the whole workgroup instead)
    {
        if (!golomb()) for (int k = 0; k < 2 * kStateBytes; ++k) st[k] = 128;
        else for (int k = 0; k < 2 * kContexts; ++k) vlc_reset(reinterpret_cast<VlcState*>(st) + k);
    }

    // `avail` bytes can be read through src (the payload and what follows it in the packet), `size` of them are the payload
    MDVT_HD uint32_t begin(Src src, uint32_t avail, uint32_t size, bool first, int coder_type, int micro, int W, int H, int nh, int nv,
                           const uint16_t* next, int planar = 0, int hs = 0, int vs = 0)
    {
        c.src = src; c.next = next;
        c.range = 0xFF00; c.overread = 0; c.pos = 2; c.end = size;
        coder = kGolomb ? coder_type : 1; run_index = 0; key = 0;
        error = false; sw = sh = 0; x0 = y0 = 0; cell = 0; csw = csh = 0;
        // the host starts the first slice's coder on the whole packet (>= 3 bytes), the others on their payload (>= 2 bytes, or refused)
        if (first ? avail < 2u : size < 2u) return kDamaged;
        c.low = ((int)src.byte(0) << 8) | (int)src.byte(1);
        if (c.low >= 0xFF00) { c.low = 0xFF00; if (!first) c.end = 2; }
        for (int k = 0; k < 64; ++k) misc[k] = 128;
        if (first) key = c.get(misc + 32);
        bool bad = false;
        const unsigned sx = (unsigned)c.symbol(misc, false, &bad), sy = (unsigned)c.symbol(misc, false, &bad);
        const unsigned cw = (unsigned)c.symbol(misc, false, &bad) + 1u, ch = (unsigned)c.symbol(misc, false, &bad) + 1u;
        if (bad || sx >= (unsigned)nh || sy >= (unsigned)nv || cw > (unsigned)nh - sx || ch > (unsigned)nv - sy) return kBadSliceHeader;
        // nh * nv slices share nh * nv cells: a slice of more than one cell overlaps another or leaves a hole (the caller checks
        // that no two slices claim the same cell, so the frame's slices tile it)
        if (cw != 1u || ch != 1u) return kBadSliceHeader;
        for (int p = 0; p < 2; ++p)
            if (c.symbol(misc, false, &bad) != 0 || bad) return kBadSliceHeader;     // quant_table_set_index: one set
        (void)c.symbol(misc, false, &bad);                                         // picture_structure, sar_num, sar_den
        (void)c.symbol(misc, false, &bad);
        (void)c.symbol(misc, false, &bad);
        if (bad) return kBadSliceHeader;
        cell = (int)(sy * (unsigned)nh + sx);
        x0 = (int)((long long)sx * W / nh); y0 = (int)((long long)sy * H / nv);
        sw = (int)((long long)(sx + 1u) * W / nh) - x0; sh = (int)((long long)(sy + 1u) * H / nv) - y0;
        if (sw < 1 || sh < 1 || sw + 2 > stride) return kBadSliceHeader;
        if (planar) { csw = (sw + (1 << hs) - 1) >> hs; csh = (sh + (1 << vs) - 1) >> vs; }
        if (golomb()) {
            if (micro > 1) { misc[33] = 129; (void)c.get(misc + 33); }             // the sentinel of ff_rac_terminate
            const uint32_t consumed = c.pos - 1u;                                  // the host's `p - start - 1`
            if (consumed > size) return kBadSliceHeader;                           // "header overruns the slice"
            gb.init(src, consumed, size - consumed);
        }
        return kOk;
    }

    // one row of `w` samples of kBits bits: `cur` the row's slot, `last` the slot of the row above; set: the context set (0 luma, 1 chroma)
    template <int kBits>
    MDVT_HD void line(int16_t* cur, int16_t* last, int w, int set)
    {
        constexpr int kMask = (1 << kBits) - 1;
        cur[-1] = last[0];
        last[w] = last[w - 1];
        int L = cur[-1], LT = last[-1], T = last[0];
        int q_lt_t = q11[(LT - T) & 0xFF];                 // (this sample's T - RT is the next one's LT - T)
        if (!golomb()) {
            uint8_t* states = st + (set ? kStateBytes : 0);
            for (int x = 0; x < w; ++x) {
                const int RT = last[x + 1];
                const int q_t_rt = q11[(T - RT) & 0xFF];
                int context = q11[(L - LT) & 0xFF] + 11 * q_lt_t + 121 * q_t_rt;
                q_lt_t = q_t_rt;
                const bool sign = context < 0;
                if (sign) context = -context;
                bool bad = false;
                int diff = c.symbol(states + (size_t)context * 32u, true, &bad);
                error |= bad;
                if (sign) diff = -diff;
                const int v = (median3(L, T, L + T - LT) + diff) & kMask;
                cur[x] = (int16_t)v;
                L = v; LT = T; T = RT;
            }
            return;
        }
        // Golomb-Rice with run mode (the host's decode_line): run_index runs on across rows (and, in the RCT's slices, planes)
        VlcState* vs = reinterpret_cast<VlcState*>(st) + (set ? kContexts : 0);
        int run_count = 0, run_mode = 0;
        for (int x = 0; x < w; ++x) {
            const int RT = last[x + 1];
            const int q_t_rt = q11[(T - RT) & 0xFF];
            int context = q11[(L - LT) & 0xFF] + 11 * q_lt_t + 121 * q_t_rt;
            q_lt_t = q_t_rt;
            const bool sign = context < 0;
            if (sign) context = -context;
            int diff;
            if (context == 0 && run_mode == 0) run_mode = 1;
            if (run_mode) {
                if (run_count == 0 && run_mode == 1) {
                    const int lr = log2_run(run_index);
                    if (gb.get(1)) {
                        run_count = 1 << lr;
                        if (x + run_count <= w) { if (run_index < kRunIndexMax) ++run_index; }
                        else stats.short_tail_run();
                        stats.run_index(run_index);
                    } else {
                        run_count = (int)gb.get(lr);
                        if (run_index) --run_index;
                        run_mode = 2;
                    }
                }
                --run_count;
                if (run_count < 0) {
                    run_mode = 0; run_count = 0;
                    diff = get_vlc_symbol<kBits>(gb, vs + context, stats);
                    if (diff >= 0) ++diff;
                } else diff = 0;
            } else diff = get_vlc_symbol<kBits>(gb, vs + context, stats);
            if (sign) diff = -diff;
            const int v = (median3(L, T, L + T - LT) + diff) & kMask;
            cur[x] = (int16_t)v;
            L = v; LT = T; T = RT;
        }
    }

    MDVT_HD void row(int y)
    {
        const int cs = y % 3, ls = (y + 2) % 3;
        for (int p = 0; p < 3; ++p)
            line<9>(lines + (size_t)(p * 3 + cs) * (size_t)stride + 1, lines + (size_t)(p * 3 + ls) * (size_t)stride + 1, sw, p ? 1 : 0);
    }

    // planar mode: row y of plane p; the run index restarts at each plane
    MDVT_HD void plane_row(int p, int y)
    {
        const int cs = y % 3, ls = (y + 2) % 3;
        if (y == 0) run_index = 0;
        line<8>(lines + (size_t)(p * 3 + cs) * (size_t)stride + 1, lines + (size_t)(p * 3 + ls) * (size_t)stride + 1, p ? csw : sw, p ? 1 : 0);
    }

    // (the host reader has no overread check on the Golomb side: c.overread counts the header's reads alone there)
    MDVT_HD uint32_t finish() const { return (error || c.overread > 4) ? kDamaged : kOk; }
};

// ---- the configuration record (RFC 9043 section 4.2), host side: is the stream in the class the entry point decodes? ----
struct PtrSrc {
    const uint8_t* p;
    MDVT_HD uint8_t byte(uint32_t k) const { return p[k]; }
};

struct StreamClass { int version, micro, nh, nv, ec, coder, intra, planar, hs, vs; };      // planar: YCbCr with log2 chroma subsampling hs, vs

// -> nullptr and *out when the stream is in the class asked for -- intra: coder_type 1, intra 1, RGB; stream: coder_type 0 or 1,
// intra 0 or 1, RGB or 8-bit YCbCr in 4:4:4, 4:2:2 or 4:2:0 --, else the reason (a static string naming the field)
inline const char* parse_stream_class(const uint8_t* data, size_t size, bool stream, StreamClass* out)
{
    if (!data || size < 6 || size > (1u << 20)) return "configuration record: missing or of an impossible size";
    const uint32_t crc = crc32_msb(0, data, size);
    uint8_t state[32];
    for (int k = 0; k < 32; ++k) state[k] = 128;
    RacDec<PtrSrc> c;
    c.init(PtrSrc{data}, (uint32_t)size, default_next_states());
    bool bad = false;
    const int version = c.symbol(state, false, &bad);
    if (bad || version != 3) return "version: only FFV1 version 3 is decoded on the device";
    c.end = c.end >= 4u ? c.end - 4u : 0u;                   // the record's CRC parity is not range-coded
    const int micro = c.symbol(state, false, &bad);
    const int coder = c.symbol(state, false, &bad);
    if (!stream) {
        if (bad || coder != 1) return "coder_type: only the range coder with the default state table (coder_type 1) is decoded on the device";
    } else {
        if (!bad && coder == 2) return "coder_type 2: a custom state-transition table is not decoded on the device";
        if (bad || (coder != 0 && coder != 1))
            return "coder_type: only Golomb-Rice (coder_type 0) and the range coder with the default state table (coder_type 1) are decoded on the device";
    }
    const int colorspace = c.symbol(state, false, &bad);
    if (!stream) {
        if (bad || colorspace != 1) return "colorspace_type: only RGB (JPEG 2000 RCT) is decoded on the device";
    } else if (bad || (colorspace != 0 && colorspace != 1))
        return "colorspace_type: only YCbCr (0) and RGB (1, the JPEG 2000 RCT) are decoded on the device";
    const int bits = c.symbol(state, false, &bad);
    if (bad || (bits != 0 && bits != 8)) return "bits_per_raw_sample: only 8 bits are decoded on the device";
    const int chroma_planes = c.get(state);
    const int hs = c.symbol(state, false, &bad), vs = c.symbol(state, false, &bad);      // (an RGB stream's are not looked at)
    if (colorspace == 0) {
        if (!chroma_planes) return "chroma_planes: a YCbCr stream without chroma planes (grey) is not decoded on the device";
        if (bad || !((hs == 0 && vs == 0) || (hs == 1 && vs == 0) || (hs == 1 && vs == 1)))
            return "log2_h_chroma_subsample / log2_v_chroma_subsample: only (0, 0), (1, 0) and (1, 1) -- yuv444p, yuv422p, yuv420p -- are decoded on the device";
    }
    if (c.get(state)) return "extra_plane: alpha planes are not decoded on the device";
    const int nh = 1 + c.symbol(state, false, &bad), nv = 1 + c.symbol(state, false, &bad);
    if (bad || nh < 1 || nv < 1 || nh > kMaxSlices || nv > kMaxSlices || nh * nv > kMaxSlices)
        return "num_h_slices / num_v_slices: 1 to 1024 slices per frame are decoded on the device";
    const int qcount = c.symbol(state, false, &bad);
    if (bad || qcount != 1) return "quant_table_set_count: only one quantisation table set is decoded on the device";
    int scale = 1;
    for (int t = 0; t < 5; ++t) {                            // the host decoder's read_quant_tables, compared with the default set
        uint8_t qs[32];
        for (int k = 0; k < 32; ++k) qs[k] = 128;
        int i = 0, v = 0;
        for (; i < 128; ++v) {
            const unsigned len = (unsigned)c.symbol(qs, false, &bad) + 1u;
            if (bad || len > (unsigned)(128 - i)) return "quantisation tables: malformed";
            for (unsigned k = 0; k < len; ++k, ++i)
                if (scale * v != (t < 3 ? scale * quant11(i) : 0))
                    return "quantisation tables: only the default 666-context set (quant11, three inputs) is decoded on the device";
        }
        scale *= 2 * v - 1;
        if (scale > 32768 || scale <= 0) return "quantisation tables: malformed";
    }
    if (scale != 11 * 11 * 11) return "quantisation tables: only the default 666-context set (quant11, three inputs) is decoded on the device";
    if (c.get(state)) return "states_coded: initial states other than 128 are not decoded on the device";
    const int ec = c.symbol(state, false, &bad);
    if (bad || (ec != 0 && ec != 1)) return "ec: unknown error-correction mode";
    const int intra = micro > 2 ? c.symbol(state, false, &bad) : 0;
    if (bad) return "configuration record: malformed symbol";
    if (!stream && !intra) return "intra: only streams whose every frame is a key frame are decoded on the device";
    if (crc != 0) return "configuration record: CRC mismatch";
    out->version = version; out->micro = micro; out->nh = nh; out->nv = nv; out->ec = ec; out->coder = coder; out->intra = intra ? 1 : 0;
    out->planar = colorspace == 0; out->hs = out->planar ? hs : 0; out->vs = out->planar ? vs : 0;
    return nullptr;
}

}  // namespace mdvt_ffv1
