// The device FFV1 decoder's core (csrc/mdvt_ffv1_core.h) compiled for the host: tests/test_video_decoder_cpu.py builds this
// program at test time (with -fsanitize=address,undefined where the compiler has the runtime) and feeds it packets.
//
//   ffv1_decode_host <jobs file> <results file>
// jobs:    u32 count, then per job u32 width, height, order, config bytes, packet bytes, then the record and the packet
// results: per job u32 status (the kernels' status words; 100 = the record is outside the device's class), u32 samples decoded,
//          then width * height * 3 bytes (zero where nothing was stored)
// The frame is decoded the way the kernels do it: slice table first, CRCs next, then slice by slice with the cell claims.  Every
// buffer is allocated at its exact size and every byte of a packet is read through a checked accessor.
#include "ffv1_host_common.h"

static uint32_t decode(int W, int H, int order, const std::vector<uint8_t>& cfg, const std::vector<uint8_t>& pkt_in, uint8_t* dst, uint32_t* samples)
{
    StreamClass sc{};
    if (parse_stream_class(cfg.data(), cfg.size(), false, &sc) || sc.nh > W || sc.nv > H) return 100;
    // the packet at its exact size on the heap: a read past it is the sanitizer's
    uint8_t* pkt = (uint8_t*)malloc(pkt_in.size() ? pkt_in.size() : 1);
    memcpy(pkt, pkt_in.data(), pkt_in.size());
    const uint32_t size = (uint32_t)pkt_in.size();
    const int n = sc.nh * sc.nv;
    std::vector<uint32_t> off((size_t)n), len((size_t)n), claims((size_t)n, 0);
    uint32_t status = walk_slices(CheckedPacket{pkt, size}, size, n, sc.ec, off.data(), len.data());
    const uint32_t trailer = sc.ec ? 8u : 3u;
    if (status == kOk && sc.ec)
        for (int i = 0; i < n; ++i)
            if (slice_crc(CheckedPacket{pkt, size}, off[i], len[i] + trailer)) status = kCrcMismatch;      // (the kernel skips the slice; here the whole frame)
    const Tables tab;
    const int stride = (W + sc.nh - 1) / sc.nh + 2;
    const int ri = order == 1 ? 2 : 0, bi = order == 1 ? 0 : 2;
    for (int i = 0; i < n && status == kOk; ++i) {
        SliceDec<CheckedSrc> d;
        d.coder = sc.coder;
        uint8_t* st = (uint8_t*)malloc(state_bytes(d.coder));
        int16_t* lines = (int16_t*)calloc((size_t)9 * stride, sizeof(int16_t));
        uint8_t* misc = (uint8_t*)malloc(64);
        d.st = st; d.lines = lines; d.misc = misc; d.q11 = tab.q11; d.stride = stride;
        d.reset_state();
        uint32_t s = d.begin(CheckedSrc{pkt + off[i], len[i] + trailer}, len[i] + trailer, len[i], i == 0, sc.coder, sc.micro, W, H, sc.nh, sc.nv, tab.next);
        if (s == kOk && i == 0 && !d.key) s = kBadSliceHeader;   // not a key frame: k_ffv1_dec_slice's verdict
        if (s == kOk) {
            CHECK(d.cell >= 0 && d.cell < n);
            if (claims[(size_t)d.cell]++) s = kBadSliceHeader;
        }
        if (s == kOk) {
            CHECK(d.x0 >= 0 && d.y0 >= 0 && d.x0 + d.sw <= W && d.y0 + d.sh <= H);
            for (int y = 0; y < d.sh; ++y) {
                d.row(y);
                *samples += 3u * (uint32_t)d.sw;
                store_row(d, y, dst, W, ri, bi);
            }
            s = d.finish();
        }
        if (s > status) status = s;
        free(st); free(lines); free(misc);
    }
    free(pkt);
    return status;
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t count = 0;
    if (!rd(in, &count, 4)) return 2;
    for (uint32_t j = 0; j < count; ++j) {
        uint32_t h[5];
        if (!rd(in, h, sizeof h) || h[0] < 1 || h[1] < 1 || h[0] > 8192 || h[1] > 8192 || h[3] > (1u << 20) || h[4] > (1u << 28)) return 2;
        std::vector<uint8_t> cfg(h[3]), pkt(h[4]), dst((size_t)h[0] * h[1] * 3, 0);
        if (!rd(in, cfg.data(), cfg.size()) || !rd(in, pkt.data(), pkt.size())) return 2;
        uint32_t res[2] = {0, 0};
        res[0] = decode((int)h[0], (int)h[1], (int)h[2], cfg, pkt, dst.data(), &res[1]);
        fwrite(res, 4, 2, out);
        fwrite(dst.data(), 1, dst.size(), out);
    }
    fclose(in);
    return fclose(out) ? 2 : 0;
}
