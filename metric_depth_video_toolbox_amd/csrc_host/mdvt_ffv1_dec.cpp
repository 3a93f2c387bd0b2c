// mdvt_ffv1_dec.cpp -- the host's FFV1 decoder, over the primitives of csrc/mdvt_ffv1_core.h.
//
// FFV1 versions 0, 1 (global header inside every key frame, one slice) and 3 (configuration record in the container's
// CodecPrivate, N slices per frame, each followed by its 24-bit size, an error-status byte and a CRC-32 parity when ec = 1);
// coder_type 0 (Golomb-Rice with run mode), 1 (range coder, default state-transition table) and 2 (custom table sent as deltas);
// colorspace_type 1 (JPEG 2000 RCT over 8-bit R, G, B, +- alpha: what FFmpeg codes for bgr0 / bgra, the pixel format OpenCV feeds
// FFV1) and colorspace_type 0 (YCbCr, 8 bits, chroma subsampled by (0, 0), (1, 0) or (1, 1): yuv444p, yuv422p, yuv420p -- FFmpeg's
// default for a movie -- converted to RGB as include/mdvt_video.h states it); key frames AND inter frames (inter frames keep the
// context states of the previous frame, so the stream is read in order).  Grey, alpha beside YCbCr and more than 8 bits are refused
// with a message.  This is the general line decoder -- up to five context inputs, several quantisation table sets, initial states --
// where the core's SliceDec is specialised to the default 666-context set.  Slices are decoded on std::threads.
#include "mdvt_ffv1_host.h"

namespace mdvt_host {

namespace {

using Rac = RacDec<PtrSrc>;

// one set of five tables, run-length coded (RFC 9043 section 4.9.? QuantizationTable)
bool read_quant_table(Rac& c, int16_t* q, int scale, int* levels)
{
    uint8_t state[kContextSize];
    memset(state, 128, sizeof state);
    int i = 0, v = 0;
    for (; i < 128; ++v) {
        bool bad = false;
        const unsigned len = (unsigned)c.symbol(state, false, &bad) + 1u;
        if (bad || len > (unsigned)(128 - i)) return false;
        for (unsigned k = 0; k < len; ++k) q[i++] = (int16_t)(scale * v);
    }
    for (i = 1; i < 128; ++i) q[256 - i] = (int16_t)-q[i];
    q[128] = (int16_t)-q[127];
    *levels = 2 * v - 1;
    return true;
}

int read_quant_tables(Rac& c, int16_t q[kMaxContextInputs][256])
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

// coder_type, with the stream's own state table when it is 2: deltas to the default one_state[], read with `state`
int read_coder_type(Rac& c, uint8_t* state, uint8_t* delta_state, Ffv1Config& f, bool* bad)
{
    const int coder = c.symbol(state, false, bad);
    const uint16_t* def = default_next_states();
    if (coder == 2) {
        uint8_t one[256];
        one[0] = 0;
        for (int i = 1; i < 256; ++i) one[i] = (uint8_t)(c.symbol(delta_state, true, bad) + (def[i] >> 8));
        custom_next_states(one, f.next);
    } else memcpy(f.next, def, sizeof f.next);
    return coder;
}

}  // namespace

int parse_config_record(const uint8_t* data, size_t size, Ffv1Config& f)
{
    if (size < 6 || size > 0xFFFFFFFFu) return fail(ERR_FORMAT, "FFV1 configuration record of %zu bytes", size);
    Rac c;
    c.init(PtrSrc{data}, (uint32_t)size, default_next_states());
    uint8_t state[kContextSize], state2[kContextSize];
    memset(state, 128, sizeof state);
    memset(state2, 128, sizeof state2);
    bool bad = false;
    f.version = c.symbol(state, false, &bad);
    if (f.version > 2) { c.end = c.end >= 4u ? c.end - 4u : 0u; f.micro = c.symbol(state, false, &bad); }     // the CRC parity is not range-coded
    f.coder = read_coder_type(c, state, state2, f, &bad);
    f.colorspace = c.symbol(state, false, &bad);
    f.bits = c.symbol(state, false, &bad);
    f.chroma_planes = c.get(state);
    f.hshift = c.symbol(state, false, &bad);
    f.vshift = c.symbol(state, false, &bad);
    f.alpha = c.get(state);
    f.nh = 1 + c.symbol(state, false, &bad);
    f.nv = 1 + c.symbol(state, false, &bad);
    f.qcount = c.symbol(state, false, &bad);
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
                    f.initial_states[i][(size_t)j * kContextSize + k] = (uint8_t)((pred + c.symbol(state2, true, &bad)) & 0xFF);
                }
        }
    }
    if (f.version > 2) {
        f.ec = c.symbol(state, false, &bad);
        if (f.micro > 2) f.intra = c.symbol(state, false, &bad);
        if (crc32_msb(0, data, size) != 0) return fail(ERR_DATA, "FFV1 configuration record: CRC mismatch");
    }
    if (bad) return fail(ERR_FORMAT, "FFV1 configuration record: malformed symbol");
    return 0;
}

namespace {

void reset_plane(const Ffv1Config& f, PlaneState& p)
{
    const int n = f.context_count[p.qidx];
    if (f.coder) {
        if (!f.initial_states[p.qidx].empty()) p.state = f.initial_states[p.qidx];
        else p.state.assign((size_t)n * kContextSize, 128);
    } else p.vlc.assign((size_t)n, fresh_vlc());
}

struct SliceDecoder {
    const Ffv1Config* f;
    Rac c;
    BitReader<PtrSrc> gb;
    NoStats stats;
    int run_index = 0;
    bool error = false;

    // sample[0] = previous line, sample[1] = the line being decoded (still holding the line two rows up: that is TT)
    template <int kBits>
    void decode_line(PlaneState& p, int w, int16_t* sample[2])
    {
        LineCtx lc{f->quant[p.qidx], f->quant[p.qidx][3][127] != 0 || f->quant[p.qidx][4][127] != 0};
        int run_count = 0, run_mode = 0;
        constexpr int mask = (1 << kBits) - 1;
        if (f->coder) {
            // the range coder's line on a copy of the coder: a local's fields stay in registers across the byte stores into the states
            Rac rc = c;
            uint8_t* states = p.state.data();
            bool bad = false;
            for (int x = 0; x < w; ++x) {
                int context = get_context(lc, sample[1] + x, sample[0] + x, sample[1] + x);
                const bool sign = context < 0;
                if (sign) context = -context;
                int diff = rc.symbol(states + (size_t)context * kContextSize, true, &bad);
                if (sign) diff = -diff;
                const int pred = median3(sample[1][x - 1], sample[0][x], sample[1][x - 1] + sample[0][x] - sample[0][x - 1]);
                sample[1][x] = (int16_t)((pred + diff) & mask);
            }
            c = rc;
            error |= bad;
            return;
        }
        for (int x = 0; x < w; ++x) {
            int context = get_context(lc, sample[1] + x, sample[0] + x, sample[1] + x);
            const bool sign = context < 0;
            if (sign) context = -context;
            int diff;
            if (context == 0 && run_mode == 0) run_mode = 1;
            if (run_mode) {
                if (run_count == 0 && run_mode == 1) {
                    const int lr = log2_run(run_index);
                    if (gb.get(1)) {
                        run_count = 1 << lr;
                        if (x + run_count <= w && run_index < kRunIndexMax) ++run_index;
                    } else {
                        run_count = (int)gb.get(lr);
                        if (run_index) --run_index;
                        run_mode = 2;
                    }
                }
                --run_count;
                if (run_count < 0) {
                    run_mode = 0; run_count = 0;
                    diff = get_vlc_symbol<kBits>(gb, &p.vlc[(size_t)context], stats);
                    if (diff >= 0) ++diff;
                } else diff = 0;
            } else diff = get_vlc_symbol<kBits>(gb, &p.vlc[(size_t)context], stats);
            if (sign) diff = -diff;
            const int pred = median3(sample[1][x - 1], sample[0][x], sample[1][x - 1] + sample[0][x] - sample[0][x - 1]);
            sample[1][x] = (int16_t)((pred + diff) & mask);
        }
    }
};

// versions 0 / 1 (RFC 9043 section 4.? "Frame" with version <= 1)
int read_frame_header(Ffv1Config& f, Rac& c, uint8_t* state)
{
    bool bad = false;
    const int v = c.symbol(state, false, &bad);
    if (bad || v > 1) return fail(ERR_UNSUPPORTED, "FFV1 frame header announces version %d inside the frame", v);
    f.version = v;
    f.coder = read_coder_type(c, state, state, f, &bad);
    f.colorspace = c.symbol(state, false, &bad);
    f.bits = f.version > 0 ? c.symbol(state, false, &bad) : 8;
    f.chroma_planes = c.get(state);
    f.hshift = c.symbol(state, false, &bad);
    f.vshift = c.symbol(state, false, &bad);
    f.alpha = c.get(state);
    f.nh = f.nv = 1; f.qcount = 1; f.ec = 0; f.intra = 0;
    f.context_count[0] = read_quant_tables(c, f.quant[0]);
    if (bad || f.context_count[0] < 0) return fail(ERR_FORMAT, "FFV1 frame header: malformed");
    f.initial_states[0].clear();
    return 0;
}

// one slice: `size` bytes at `data` are its range-coded / Golomb-coded payload (trailer already cut off).  `started`: the frame's
// coder behind the key-frame bit (and the frame header of versions 0 / 1), for the first slice, which begins at the packet's start
int decode_slice(Decoder& d, int index, const uint8_t* data, uint32_t size, bool key, uint8_t* dst, size_t pitch, int order, const Rac* started)
{
    const Ffv1Config& f = d.f;
    const int W = d.W, H = d.H;
    SliceDecoder sd;
    sd.f = &f;
    if (started) { sd.c = *started; sd.c.end = size; }
    else if (!sd.c.init(PtrSrc{data}, size, f.next)) return fail(ERR_DATA, "FFV1 slice %d: %zu bytes", index, (size_t)size);
    sd.c.next = f.next;
    SliceState& ss = d.slices[(size_t)index];
    int x0 = 0, y0 = 0, sw = W, sh = H;
    if (f.version >= 3) {
        uint8_t state[kContextSize];
        memset(state, 128, sizeof state);
        bool bad = false;
        const unsigned sx = (unsigned)sd.c.symbol(state, false, &bad), sy = (unsigned)sd.c.symbol(state, false, &bad);
        const unsigned cw = (unsigned)sd.c.symbol(state, false, &bad) + 1u, ch = (unsigned)sd.c.symbol(state, false, &bad) + 1u;
        if (bad || sx >= (unsigned)f.nh || sy >= (unsigned)f.nv || sx + cw > (unsigned)f.nh || sy + ch > (unsigned)f.nv)
            return fail(ERR_DATA, "FFV1 slice %d: bad slice position", index);
        x0 = (int)((int64_t)sx * W / f.nh); y0 = (int)((int64_t)sy * H / f.nv);
        sw = (int)((int64_t)(sx + cw) * W / f.nh) - x0; sh = (int)((int64_t)(sy + ch) * H / f.nv) - y0;
        for (int p = 0; p < f.plane_count(); ++p) {
            const int idx = sd.c.symbol(state, false, &bad);
            if (bad || idx < 0 || idx >= f.qcount) return fail(ERR_DATA, "FFV1 slice %d: bad quantisation table index", index);
            if (ss.plane[p].qidx != idx) { ss.plane[p].qidx = idx; ss.plane[p].state.clear(); ss.plane[p].vlc.clear(); }
        }
        (void)sd.c.symbol(state, false, &bad);      // picture_structure
        (void)sd.c.symbol(state, false, &bad);      // sar_num
        (void)sd.c.symbol(state, false, &bad);      // sar_den
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
        const uint32_t consumed = sd.c.pos - 1u;            // the bit stream starts on the last byte the range coder took in
        if (consumed > size) return fail(ERR_DATA, "FFV1 slice %d: header overruns the slice", index);
        sd.gb.init(PtrSrc{data}, consumed, size - consumed);
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
                sd.decode_line<8>(ss.plane[p ? 1 : 0], w, sample);
                for (int x = 0; x < w; ++x) pl[p][(size_t)y * (size_t)w + (size_t)x] = (uint8_t)sample[1][x];
            }
        }
        for (int y = 0; y < sh; ++y) {
            uint8_t* o = dst + (size_t)(y0 + y) * pitch + (size_t)x0 * 3;
            const uint8_t* ly = pl[0].data() + (size_t)y * (size_t)sw;
            const uint8_t* lu = pl[1].data() + (size_t)(y >> vs) * (size_t)cw;
            const uint8_t* lv = pl[2].data() + (size_t)(y >> vs) * (size_t)cw;
            for (int x = 0; x < sw; ++x) store_ycbcr_pixel(ly[x], lu[x >> hs], lv[x >> hs], o + 3 * x, ri, 1, bi);
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
            sd.decode_line<9>(ps, sw, sample[p]);                        // 8-bit RGB: every plane, alpha included, is coded with 9 bits
        }
        uint8_t* o = dst + (size_t)(y0 + y) * pitch + (size_t)x0 * 3;
        for (int x = 0; x < sw; ++x) store_rct_pixel(sample[0][1][x], sample[1][1][x], sample[2][1][x], o + 3 * x, ri, 1, bi);
    }
    if (sd.error || sd.c.overread > 4) return fail(ERR_DATA, "FFV1 slice %d: bitstream damaged (overread %d)", index, sd.c.overread);
    return 0;
}

}  // namespace

int Decoder::check_supported() const
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

int Decoder::decode_frame(const uint8_t* pkt, size_t size, uint8_t* dst, size_t pitch, int order, int threads)
{
    if (size < 3 || size > 0xFFFFFFFFu) return fail(ERR_DATA, "FFV1 packet of %zu bytes", size);
    Rac c;
    c.init(PtrSrc{pkt}, (uint32_t)size, default_next_states());
    uint8_t keystate = 128;
    const bool key = c.get(&keystate) != 0;
    if (key) {
        if (!have_config || f.version < 2) {
            uint8_t state[kContextSize];
            memset(state, 128, sizeof state);
            int rc = read_frame_header(f, c, state);
            if (rc) return rc;
            have_config = true;
        }
        int rc = check_supported();
        if (rc) return rc;
        key_frame_ok = true;
    } else if (!key_frame_ok) return fail(ERR_DATA, "FFV1: the stream does not start with a key frame");
    const int n = f.version >= 3 ? f.nh * f.nv : 1;
    if ((int)slices.size() != n) slices.assign((size_t)n, SliceState());
    // Slice extents, from the end of the packet (RFC 9043 section 4.? slice footers).  The core's walk_slices does this arithmetic for
    // the device; this walk is the host's own because it checks each slice's CRC on the way and says which check refused the packet.
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
    return run_slices(n, threads, [&](int i) {
        return decode_slice(*this, i, pkt + ext[(size_t)i].first, (uint32_t)ext[(size_t)i].second, key, dst, pitch, order, i == 0 ? &c : nullptr);
    });
}

}  // namespace mdvt_host
