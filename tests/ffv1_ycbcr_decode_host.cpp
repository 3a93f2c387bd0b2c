// The device FFV1 stream decoder's core with its planar mode (csrc/mdvt_ffv1_core.h: SliceDec::plane_row, planar_store_row, the
// stream class of the parser with YCbCr in it) compiled for the host: tests/test_ffv1_ycbcr_cpu.py builds this program at test time
// (plain, and with -fsanitize=address,undefined where the compiler has the runtime), runs it directly and feeds it YCbCr streams.
//
//   ffv1_ycbcr_decode_host <jobs file> <results file>
// The files are those of tests/ffv1_stream_decode_host.cpp (verdict 100: the record, or its slice grid on this frame size, is
// outside the class).  The stream is decoded the way the kernels do it: the walk, then for every key frame and slice one chain
// through the run's frames; a YCbCr slice is its plane rows in coding order, each handed to planar_store_row for 64 lanes in turn,
// which parks Y and Cb in the slice's own pixels of the stored frame and converts when a row of Cr is there.  Every buffer is
// allocated at its exact size and every byte of a packet is read through a checked accessor.
#include "ffv1_host_common.h"

struct Counters {
    uint32_t escapes = 0, halvings = 0, max_run_index = 0, short_tail_runs = 0;
    void escape() { ++escapes; }
    void halving() { ++halvings; }
    void run_index(int r) { CHECK(r >= 0 && r <= kRunIndexMax); if ((uint32_t)r > max_run_index) max_run_index = (uint32_t)r; }
    void short_tail_run() { ++short_tail_runs; }
};

struct Packet { uint8_t* p; uint32_t size; };           // on the heap at its exact size: a read past it is the sanitizer's

static void raise_status(std::vector<uint32_t>& status, size_t k, uint32_t v) { if (v > status[k]) status[k] = v; }

static bool grid_aligned(const StreamClass& sc, int W, int H)
{
    for (int sx = 0; sx < sc.nh; ++sx) if (((long long)sx * W / sc.nh) & ((1 << sc.hs) - 1)) return false;
    for (int sy = 0; sy < sc.nv; ++sy) if (((long long)sy * H / sc.nv) & ((1 << sc.vs) - 1)) return false;
    return true;
}

static uint32_t decode(int W, int H, int order, int first_out, const std::vector<uint8_t>& cfg, const std::vector<Packet>& pk,
                       std::vector<uint32_t>& status, uint8_t* dst, Counters& total)
{
    StreamClass sc{};
    if (parse_stream_class(cfg.data(), cfg.size(), true, &sc) || sc.nh > W || sc.nv > H) return 100;
    if (sc.planar && !grid_aligned(sc, W, H)) return 100;
    const int n = (int)pk.size(), spf = sc.nh * sc.nv;
    const uint32_t trailer = sc.ec ? 8u : 3u;
    std::vector<uint32_t> off((size_t)n * spf), len((size_t)n * spf), claims((size_t)n * spf, 0), kind((size_t)n);
    for (int f = 0; f < n; ++f) {                            // k_ffv1_stream_walk
        status[(size_t)f] = walk_slices(CheckedPacket{pk[f].p, pk[f].size}, pk[f].size, spf, sc.ec, &off[(size_t)f * spf], &len[(size_t)f * spf]);
        kind[(size_t)f] = status[(size_t)f] != kOk ? kFrameBad : key_frame_bit(CheckedPacket{pk[f].p, pk[f].size}(0), CheckedPacket{pk[f].p, pk[f].size}(1)) ? kFrameKey : kFrameInter;
    }
    for (int j = 0; j < n && kind[(size_t)j] != kFrameKey; ++j) raise_status(status, (size_t)j, kNoKeyFrame);
    const Tables tab;
    const int stride = (W + sc.nh - 1) / sc.nh + 2;
    const int ri = order == 1 ? 2 : 0, bi = order == 1 ? 0 : 2;
    const size_t pitch = (size_t)W * 3;
    for (int f0 = 0; f0 < n; ++f0) {
        if (kind[(size_t)f0] != kFrameKey) continue;
        for (int si = 0; si < spf; ++si) {                   // one chain: k_ffv1_stream_chain
            SliceDec<CheckedSrc, true, Counters> d;
            d.coder = sc.coder;
            uint8_t* st = (uint8_t*)malloc(state_bytes(d.coder));
            int16_t* lines = (int16_t*)malloc((size_t)9 * stride * sizeof(int16_t));
            uint8_t* misc = (uint8_t*)malloc(64);
            d.st = st; d.lines = lines; d.misc = misc; d.q11 = tab.q11; d.stride = stride;
            d.reset_state();
            int f = f0;
            uint32_t flag = kOk;
            for (; f < n; ++f) {
                if (f > f0 && kind[(size_t)f] == kFrameKey) break;
                if (kind[(size_t)f] == kFrameBad) { flag = kBadPacket; break; }
                const size_t i = (size_t)f * spf + (size_t)si;
                CHECK((size_t)off[i] + len[i] + trailer <= pk[f].size);
                const uint8_t* data = pk[f].p + off[i];
                if (sc.ec && slice_crc(CheckedPacket{pk[f].p, pk[f].size}, off[i], len[i] + trailer)) { flag = kCrcMismatch; break; }
                memset(lines, 0, (size_t)9 * stride * sizeof(int16_t));
                uint32_t s = d.begin(CheckedSrc{data, len[i] + trailer}, len[i] + trailer, len[i], si == 0, sc.coder, sc.micro, W, H, sc.nh, sc.nv, tab.next,
                                     sc.planar, sc.hs, sc.vs);
                if (s == kOk) {
                    CHECK(d.cell >= 0 && d.cell < spf);
                    if (claims[(size_t)f * spf + (size_t)d.cell]++) s = kBadSliceHeader;
                }
                if (s != kOk) { flag = s; break; }
                CHECK(d.x0 >= 0 && d.y0 >= 0 && d.x0 + d.sw <= W && d.y0 + d.sh <= H);
                uint8_t* frame = f >= first_out ? dst + (size_t)(f - first_out) * pitch * H : nullptr;
                if (!sc.planar) {
                    for (int y = 0; y < d.sh; ++y) {
                        d.row(y);
                        CHECK(d.run_index >= 0 && d.run_index <= kRunIndexMax);
                        if (frame) store_row(d, y, frame, W, ri, bi);
                    }
                } else {
                    CHECK(d.csw == (d.sw + (1 << sc.hs) - 1) >> sc.hs && d.csh == (d.sh + (1 << sc.vs) - 1) >> sc.vs);
                    CHECK(((d.csw - 1) << sc.hs) < d.sw && ((d.csh - 1) << sc.vs) < d.sh);
                    for (int r = 0; r < d.sh + 2 * d.csh; ++r) {           // the plane rows in coding order, as ffv1_decode_rows_planar
                        const int p = r < d.sh ? 0 : r < d.sh + d.csh ? 1 : 2, y = r < d.sh ? r : r < d.sh + d.csh ? r - d.sh : r - d.sh - d.csh;
                        d.plane_row(p, y);
                        CHECK(d.run_index >= 0 && d.run_index <= kRunIndexMax);
                        if (frame)
                            for (int lane = 0; lane < 64; ++lane)
                                planar_store_row(lines + (size_t)(p * 3 + y % 3) * stride + 1, p, y, frame + (size_t)d.y0 * pitch + (size_t)d.x0 * 3, pitch,
                                                 d.sw, d.sh, d.csw, sc.hs, sc.vs, ri, bi, lane, 64);
                    }
                }
                s = d.finish();
                if (s != kOk) { flag = s; break; }
            }
            if (flag != kOk) {
                raise_status(status, (size_t)f, flag);
                for (int j = f + 1; j < n && kind[(size_t)j] != kFrameKey; ++j) raise_status(status, (size_t)j, kBrokenRun);
            }
            total.escapes += d.stats.escapes; total.halvings += d.stats.halvings; total.short_tail_runs += d.stats.short_tail_runs;
            if (d.stats.max_run_index > total.max_run_index) total.max_run_index = d.stats.max_run_index;
            free(st); free(lines); free(misc);
        }
    }
    return 0;
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
        uint32_t h[6];
        if (!rd(in, h, sizeof h) || h[0] < 1 || h[1] < 1 || h[0] > 8192 || h[1] > 8192 || h[4] > (1u << 20) || h[5] < 1 || h[5] > 4096 || h[3] >= h[5]) return 2;
        std::vector<uint8_t> cfg(h[4]);
        if (!rd(in, cfg.data(), cfg.size())) return 2;
        std::vector<Packet> pk;
        for (uint32_t k = 0; k < h[5]; ++k) {
            uint32_t size = 0;
            if (!rd(in, &size, 4) || size > (1u << 28)) return 2;
            Packet p{(uint8_t*)malloc(size ? size : 1), size};
            if (!rd(in, p.p, size)) return 2;
            pk.push_back(p);
        }
        const size_t frame = (size_t)h[0] * h[1] * 3;
        std::vector<uint8_t> dst(frame * (h[5] - h[3]), 0);
        std::vector<uint32_t> status(h[5], 0);
        Counters total;
        uint32_t res[5] = {decode((int)h[0], (int)h[1], (int)h[2], (int)h[3], cfg, pk, status, dst.data(), total), 0, 0, 0, 0};
        res[1] = total.escapes; res[2] = total.halvings; res[3] = total.max_run_index; res[4] = total.short_tail_runs;
        fwrite(res, 4, 5, out);
        if (res[0] == 0) {
            fwrite(status.data(), 4, status.size(), out);
            fwrite(dst.data(), 1, dst.size(), out);
        }
        for (auto& p : pk) free(p.p);
    }
    fclose(in);
    return fclose(out) ? 2 : 0;
}
