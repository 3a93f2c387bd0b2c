// tools/ffv1_ycbcr_writer.cpp -- makes YCbCr FFV1 streams at full size in reasonable time, for measurements (tools/ffv1_bench.py
// --pix-fmt): version 3.4, Golomb-Rice with run mode, intra = 0, a key frame every `gop` frames, CRC-32 parities, 8 bits, chroma
// subsampled by 2^hs x 2^vs -- the class FFmpeg writes by default for a movie.  NOT a product writer: the library writes RGB only.
// It is built on the library's own encoder parts (mdvt_ffv1_host.h: the Golomb-Rice slice start, line encoder and slice closing,
// compiled together with csrc_host/mdvt_ffv1_enc.cpp), and is byte for byte tests/ffv1_ycbcr_ref.py's Encoder
// (tests/test_ffv1_ycbcr_cpu.py).
//
//   ffv1_ycbcr_writer <planes file> <W> <H> <frames> <hs> <vs> <nh> <nv> <gop> <out file>
// planes file: per frame the Y plane (W x H bytes), then Cb and Cr (ceil(W / 2^hs) x ceil(H / 2^vs) bytes each)
// out file:    u32 bytes of the configuration record, the record, then per frame u32 bytes of the packet and the packet
#include "../metric_depth_video_toolbox_amd/csrc_host/mdvt_ffv1_host.h"

#include <stdlib.h>

using namespace mdvt_host;

namespace {

struct PlaneView { const uint8_t* p; int w, h; size_t pitch; };

// one plane of a slice: 8-bit samples, the run index restarting with the plane
void encode_plane(BitWriter& bw, std::vector<VlcState>& vlc, const PlaneView& pl, std::vector<int16_t>& buf)
{
    std::fill(buf.begin(), buf.end(), (int16_t)0);
    int16_t* sample[2] = {buf.data() + 3, buf.data() + buf.size() / 2 + 3};
    int run_index = 0;
    for (int y = 0; y < pl.h; ++y) {
        std::swap(sample[0], sample[1]);
        int16_t* cur = sample[1];
        int16_t* last = sample[0];
        const uint8_t* src = pl.p + (size_t)y * pl.pitch;
        for (int x = 0; x < pl.w; ++x) cur[x] = src[x];
        cur[-1] = last[0];
        last[pl.w] = last[pl.w - 1];
        encode_line_golomb<8>(bw, vlc.data(), cur, last, pl.w, run_index);
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 11) { fprintf(stderr, "usage: %s planes W H frames hs vs nh nv gop out\n", argv[0]); return 2; }
    const int W = atoi(argv[2]), H = atoi(argv[3]), N = atoi(argv[4]), hs = atoi(argv[5]), vs = atoi(argv[6]), nh = atoi(argv[7]), nv = atoi(argv[8]),
              gop = atoi(argv[9]);
    if (W < 1 || H < 1 || N < 1 || hs < 0 || hs > 1 || vs < 0 || vs > 1 || nh < 1 || nv < 1 || nh > W || nv > H || gop < 1) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[10], "wb");
    if (!in || !out) return 2;
    const int CW = (W + (1 << hs) - 1) >> hs, CH = (H + (1 << vs) - 1) >> vs;
    std::vector<uint8_t> Y((size_t)W * H), C[2] = {std::vector<uint8_t>((size_t)CW * CH), std::vector<uint8_t>((size_t)CW * CH)};
    const std::vector<uint8_t> rec = make_config_record(nh, nv, 0, 0, 0, hs, vs);
    const uint32_t rs = (uint32_t)rec.size();
    fwrite(&rs, 4, 1, out); fwrite(rec.data(), 1, rec.size(), out);
    std::vector<GolombSliceState> states((size_t)nh * nv);
    std::vector<int16_t> buf((size_t)2 * (W + 6));
    for (int f = 0; f < N; ++f) {
        if (fread(Y.data(), 1, Y.size(), in) != Y.size() || fread(C[0].data(), 1, C[0].size(), in) != C[0].size() ||
            fread(C[1].data(), 1, C[1].size(), in) != C[1].size()) return 2;
        const bool key = f % gop == 0;
        std::vector<uint8_t> packet;
        for (int i = 0; i < nh * nv; ++i) {
            const int sx = i % nh, sy = i / nh;
            const int x0 = (int)((int64_t)sx * W / nh), y0 = (int)((int64_t)sy * H / nv);
            const int sw = (int)((int64_t)(sx + 1) * W / nh) - x0, sh = (int)((int64_t)(sy + 1) * H / nv) - y0;
            if ((x0 & ((1 << hs) - 1)) || (y0 & ((1 << vs) - 1))) { fprintf(stderr, "slice grid off the chroma grid\n"); return 2; }
            std::vector<uint8_t> sl = golomb_slice_start(sx, sy, i == 0, key);
            GolombSliceState& ss = states[(size_t)i];
            begin_golomb_run(ss, key);
            BitWriter bw;
            const int cw = (sw + (1 << hs) - 1) >> hs, ch = (sh + (1 << vs) - 1) >> vs;
            encode_plane(bw, ss.vlc[0], PlaneView{Y.data() + (size_t)y0 * W + x0, sw, sh, (size_t)W}, buf);
            for (int p = 0; p < 2; ++p)
                encode_plane(bw, ss.vlc[1], PlaneView{C[p].data() + (size_t)(y0 >> vs) * CW + (x0 >> hs), cw, ch, (size_t)CW}, buf);
            bw.flush();
            sl.insert(sl.end(), bw.out.begin(), bw.out.end());
            if (sl.size() >= (1u << 24)) { fprintf(stderr, "a slice of %zu bytes: use more slices\n", sl.size()); return 2; }
            close_slice(sl);
            packet.insert(packet.end(), sl.begin(), sl.end());
        }
        const uint32_t ps = (uint32_t)packet.size();
        fwrite(&ps, 4, 1, out); fwrite(packet.data(), 1, packet.size(), out);
    }
    fclose(in);
    return fclose(out) ? 2 : 0;
}
