// mdvt_ffv1_enc.cpp -- the host's FFV1 encoders: version 3.4, RGB colour space (JPEG 2000 RCT), 8 bits, slices_h x slices_v slices,
// ec = 1; the quantisation tables FFmpeg's encoder uses for 8-bit input (quant11, context model 0: 666 contexts).  Two classes:
//   encode_frame          coder_type 1 (range coder, default state table), intra-only: what mdvt_video_create writes
//   encode_frame_golomb   coder_type 0 (Golomb-Rice with run mode), intra = 0, a key frame every `gop` frames -- what FFmpeg writes by
//                         default for 8-bit RGB, the opt-in stream class of include/mdvt_video_stream.h.  Byte for byte the independent
//                         restatement ffv1_ref.py's StreamEncoder(Params(coder=0, intra=0, nh, nv), W, H, gop).
// Slices are encoded on std::threads.  The decoding halves of these coders are csrc/mdvt_ffv1_core.h's.
#include "mdvt_ffv1_host.h"

namespace mdvt_host {

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Range coder (RFC 9043 section 3.8.1): binary, adaptive 8-bit states, byte-wise renormalisation
// ---------------------------------------------------------------------------------------------------------------------
// The core's default state table split by the bit.  The encoder knows its bit before it looks the next state up, and with two byte
// tables a 1920 x 1080 frame encodes about 7 % faster than through the decoder's combined table (measured both ways).
const struct SplitStates {
    uint8_t zero[256], one[256];
    SplitStates()
    {
        const uint16_t* next = default_next_states();
        for (int k = 0; k < 256; ++k) { zero[k] = (uint8_t)next[k]; one[k] = (uint8_t)(next[k] >> 8); }
    }
} g_states;

struct RacEnc {
    std::vector<uint8_t> out;           // storage; [0, size()) is the stream so far
    uint8_t* w = nullptr;               // write pointer into `out` (ensure() keeps room ahead of it)
    int low = 0, range = 0xFF00;
    int outstanding_count = 0, outstanding_byte = -1;
    const SplitStates* tab = &g_states;
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

// the range-coded integer binarisation (RFC 9043 section 3.8.1.2): 32 states per context
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

inline int fold(int diff, int bits) { const int m = 1 << (bits - 1); return ((diff + m) & ((1 << bits) - 1)) - m; }

// the writing half of the core's get_vlc_symbol
template <int kBits>
inline void put_vlc_symbol(BitWriter& bw, VlcState& st, int diff)
{
    const int v = fold(diff - st.bias, kBits);
    int i = st.count, k = 0;
    while (i < st.error_sum) { ++k; i += i; }
    const int code = v ^ ((2 * st.drift + st.count) >> 31);
    const unsigned u = code >= 0 ? 2u * (unsigned)code : 2u * (unsigned)(-code) - 1u;
    if ((u >> k) < 12u) bw.put((int)(u >> k) + k + 1, (1u << k) + (u & ((1u << k) - 1u)));
    else bw.put(12 + kBits, u - 11u);
    // update_vlc_state, as get_vlc_symbol does it
    int drift = st.drift + v, count = st.count;
    int es = st.error_sum + (v < 0 ? -v : v);
    if (count == 128) { count >>= 1; drift >>= 1; es >>= 1; }
    ++count;
    if (drift <= -count) { st.bias = (int8_t)std::max(st.bias - 1, -128); drift = std::max(drift + count, -count + 1); }
    else if (drift > 0) { st.bias = (int8_t)std::min(st.bias + 1, 127); drift = std::min(drift - count, 0); }
    st.drift = (int16_t)drift; st.count = (uint8_t)count; st.error_sum = (uint16_t)es;
}

struct EncoderTables {
    int16_t q[kMaxContextInputs][256];
    EncoderTables()
    {
        for (int i = 0; i < 256; ++i) {
            q[0][i] = (int16_t)quant11(i);
            q[1][i] = (int16_t)(11 * quant11(i));
            q[2][i] = (int16_t)(11 * 11 * quant11(i));
            q[3][i] = q[4][i] = 0;
        }
    }
};
const EncoderTables g_enc_tables;

void write_quant_table(RacEnc& c, const int16_t* q)
{
    uint8_t state[kContextSize];
    memset(state, 128, sizeof state);
    int last = 0, i;
    for (i = 1; i < 128; ++i)
        if (q[i] != q[i - 1]) { put_symbol(c, state, i - last - 1, false); last = i; }
    put_symbol(c, state, i - last - 1, false);
}

void push_be32(std::vector<uint8_t>& out, uint32_t v)
{
    out.push_back((uint8_t)(v >> 24)); out.push_back((uint8_t)(v >> 16)); out.push_back((uint8_t)(v >> 8)); out.push_back((uint8_t)v);
}

// a slice's start: the frame's key-frame bit (key_bit >= 0: the first slice) and the nine symbols of the slice header
void put_slice_header(RacEnc& c, int sx, int sy, int key_bit)
{
    c.init();
    c.ensure(1024);
    if (key_bit >= 0) { uint8_t keystate = 128; c.put(&keystate, key_bit); }
    uint8_t hstate[kContextSize];
    memset(hstate, 128, sizeof hstate);
    // position, size - 1 in slice units, the table set of the luma and of the chroma planes, progressive, unknown aspect ratio
    const int header[9] = {sx, sy, 0, 0, 0, 0, 3, 0, 0};
    for (int v : header) put_symbol(c, hstate, v, false);
}

// slice (sx, sy) of the nh x nv grid over a W x H frame, and its three planes x two lines of RCT samples
struct RctSlice {
    int x0, y0, sw, sh, ri, bi;
    std::vector<int16_t> buf;
    int16_t* sample[3][2];              // [p][0] the previous line, [p][1] the one being coded
    RctSlice(int W, int H, int nh, int nv, int sx, int sy, int order)
    {
        x0 = (int)((int64_t)sx * W / nh); y0 = (int)((int64_t)sy * H / nv);
        sw = (int)((int64_t)(sx + 1) * W / nh) - x0; sh = (int)((int64_t)(sy + 1) * H / nv) - y0;
        ri = order == MDVT_VIDEO_BGR ? 2 : 0; bi = order == MDVT_VIDEO_BGR ? 0 : 2;
        buf.assign((size_t)3 * 2 * (size_t)(sw + 6), 0);
        for (int p = 0; p < 3; ++p)
            for (int k = 0; k < 2; ++k) sample[p][k] = buf.data() + ((size_t)p * 2 + (size_t)k) * (size_t)(sw + 6) + 3;
    }
    // row y of the slice: the JPEG 2000 RCT of its pixels into the three current lines, and the lines' edges for the predictor
    void load_row(const uint8_t* src, size_t pitch, int y)
    {
        const uint8_t* s = src + (size_t)(y0 + y) * pitch + (size_t)x0 * 3;
        for (int p = 0; p < 3; ++p) std::swap(sample[p][0], sample[p][1]);
        for (int x = 0; x < sw; ++x) {
            int r = s[3 * x + ri], g = s[3 * x + 1], b = s[3 * x + bi];
            b -= g; r -= g;
            g += (b + r) >> 2;
            sample[0][1][x] = (int16_t)g; sample[1][1][x] = (int16_t)(b + 256); sample[2][1][x] = (int16_t)(r + 256);
        }
        for (int p = 0; p < 3; ++p) {
            sample[p][1][-1] = sample[p][0][0];
            sample[p][0][sw] = sample[p][0][sw - 1];
        }
    }
};

// a sample's context and its folded difference to the predictor, sign-flipped with the context
template <int kBits>
inline int context_and_diff(const int16_t* cur, const int16_t* last, int x, int* diff)
{
    const LineCtx lc{g_enc_tables.q, false};
    int context = get_context(lc, cur + x, last + x, cur + x);
    int d = cur[x] - median3(cur[x - 1], last[x], cur[x - 1] + last[x] - last[x - 1]);
    if (context < 0) { context = -context; d = -d; }
    *diff = fold(d, kBits);
    return context;
}

void encode_slice(int W, int H, int nh, int nv, int sx, int sy, const uint8_t* src, size_t pitch, int order, bool first, std::vector<uint8_t>& out)
{
    RctSlice sl(W, H, nh, nv, sx, sy, order);
    RacEnc c;
    put_slice_header(c, sx, sy, first ? 1 : -1);                       // every frame is a key frame
    std::vector<uint8_t> st[2];
    st[0].assign((size_t)kContexts * kContextSize, 128);
    st[1].assign((size_t)kContexts * kContextSize, 128);
    const int sw = sl.sw, sh = sl.sh;
    for (int y = 0; y < sh; ++y) {
        sl.load_row(src, pitch, y);
        c.ensure((size_t)sw * 3 * 24);             // a sample is at most 23 binary decisions
        for (int p = 0; p < 3; ++p) {
            const int16_t* cur = sl.sample[p][1];
            const int16_t* last = sl.sample[p][0];
            uint8_t* states = st[(p + 1) / 2].data();
            for (int x = 0; x < sw; ++x) {
                int diff;
                const int context = context_and_diff<9>(cur, last, x, &diff);
                put_symbol(c, states + (size_t)context * kContextSize, diff, true);
            }
        }
    }
    c.terminate(true);
    out = c.out;
    close_slice(out);
}

void encode_slice_golomb(int W, int H, int nh, int nv, int sx, int sy, const uint8_t* src, size_t pitch, int order, bool first, bool key,
                         GolombSliceState& ss, std::vector<uint8_t>& out)
{
    RctSlice sl(W, H, nh, nv, sx, sy, order);
    out = golomb_slice_start(sx, sy, first, key);
    begin_golomb_run(ss, key);
    BitWriter bw;
    bw.out.reserve((size_t)sl.sw * sl.sh * 3);
    int run_index = 0;
    for (int y = 0; y < sl.sh; ++y) {
        sl.load_row(src, pitch, y);
        for (int p = 0; p < 3; ++p) encode_line_golomb<9>(bw, ss.vlc[(p + 1) / 2].data(), sl.sample[p][1], sl.sample[p][0], sl.sw, run_index);
    }
    bw.flush();
    out.insert(out.end(), bw.out.begin(), bw.out.end());
    close_slice(out);
}

// the frame's packet from its slices
int join_slices(const std::vector<std::vector<uint8_t>>& parts, std::vector<uint8_t>& packet)
{
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

}  // namespace

std::vector<uint8_t> make_config_record(int nh, int nv, int coder, int intra, int colorspace, int hshift, int vshift)
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
    push_be32(out, crc32_msb(0, out.data(), out.size()));
    return out;
}

void close_slice(std::vector<uint8_t>& out)
{
    const size_t payload = out.size();
    out.push_back((uint8_t)(payload >> 16)); out.push_back((uint8_t)(payload >> 8)); out.push_back((uint8_t)payload);
    out.push_back(0);                                                                 // error_status
    push_be32(out, crc32_msb(0, out.data(), out.size()));
}

std::vector<uint8_t> golomb_slice_start(int sx, int sy, bool first, bool key)
{
    RacEnc c;
    put_slice_header(c, sx, sy, first ? (key ? 1 : 0) : -1);
    c.terminate(true);                                          // the sentinel bit: the bit stream starts behind the range coder's bytes
    return std::move(c.out);
}

void begin_golomb_run(GolombSliceState& ss, bool key)
{
    if (key || ss.vlc[0].empty())
        for (auto& v : ss.vlc) v.assign((size_t)kContexts, fresh_vlc());
}

template <int kBits>
void encode_line_golomb(BitWriter& bw, VlcState* vlc, const int16_t* cur, const int16_t* last, int w, int& run_index)
{
    auto flush_run = [&](int& run_count) {                      // whole runs of the current length: a one bit each
        while (run_count >= (1 << log2_run(run_index))) { run_count -= 1 << log2_run(run_index); if (run_index < kRunIndexMax) ++run_index; bw.put(1, 1); }
    };
    int run_count = 0, run_mode = 0;
    for (int x = 0; x < w; ++x) {
        int diff;
        const int context = context_and_diff<kBits>(cur, last, x, &diff);
        if (context == 0) run_mode = 1;
        if (run_mode) {
            if (diff) {
                flush_run(run_count);
                bw.put(1 + log2_run(run_index), (uint32_t)run_count);
                if (run_index) --run_index;
                run_count = 0; run_mode = 0;
                if (diff > 0) --diff;
            } else ++run_count;
        }
        if (run_mode == 0) put_vlc_symbol<kBits>(bw, vlc[(size_t)context], diff);
    }
    if (run_mode) {
        flush_run(run_count);
        if (run_count) bw.put(1, 1);
    }
}
template void encode_line_golomb<8>(BitWriter&, VlcState*, const int16_t*, const int16_t*, int, int&);
template void encode_line_golomb<9>(BitWriter&, VlcState*, const int16_t*, const int16_t*, int, int&);

int encode_frame(int W, int H, int nh, int nv, const uint8_t* src, size_t pitch, int order, int threads, std::vector<uint8_t>& packet)
{
    const int n = nh * nv;
    std::vector<std::vector<uint8_t>> parts((size_t)n);
    const int rc = run_slices(n, threads, [&](int i) { encode_slice(W, H, nh, nv, i % nh, i / nh, src, pitch, order, i == 0, parts[(size_t)i]); return 0; });
    return rc ? rc : join_slices(parts, packet);
}

int encode_frame_golomb(int W, int H, int nh, int nv, const uint8_t* src, size_t pitch, int order, int threads, bool key,
                        std::vector<GolombSliceState>& states, std::vector<uint8_t>& packet)
{
    const int n = nh * nv;
    states.resize((size_t)n);
    std::vector<std::vector<uint8_t>> parts((size_t)n);
    const int rc = run_slices(n, threads, [&](int i) {
        encode_slice_golomb(W, H, nh, nv, i % nh, i / nh, src, pitch, order, i == 0, key, states[(size_t)i], parts[(size_t)i]);
        return 0;
    });
    return rc ? rc : join_slices(parts, packet);
}

}  // namespace mdvt_host
