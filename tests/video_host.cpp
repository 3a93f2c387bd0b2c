// The host codec (csrc_host/) as a stand-alone program, for a run under the sanitizers (tests/test_video_host_cpu.py compiles it
// together with the library's sources): round trips through both writers and the reader, and two damaged Matroska files.
//   video_host <scratch directory>
// Prints one line per case; exit status 0 when every expectation holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mdvt_video.h"
#include "mdvt_video_stream.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED: %s (line %d): %s\n", #c, __LINE__, mdvt_video_last_error()); exit(1); } } while (0)

static std::vector<uint8_t> frame_of(int W, int H, int k, bool flat)
{
    std::vector<uint8_t> f((size_t)W * H * 3);
    uint32_t s = 12345u + (uint32_t)k * 977u;
    for (size_t i = 0; i < f.size(); ++i) {
        s = s * 1664525u + 1013904223u;
        f[i] = flat ? (uint8_t)(40 + 10 * k) : (uint8_t)((i / 3 % (size_t)W) * 5 + (s >> 28));       // a ramp with a little noise
    }
    return f;
}

static std::vector<uint8_t> slurp(const std::string& path)
{
    FILE* f = fopen(path.c_str(), "rb");
    CHECK(f);
    std::vector<uint8_t> d;
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) d.insert(d.end(), buf, buf + n);
    fclose(f);
    return d;
}

static void spit(const std::string& path, const uint8_t* p, size_t n)
{
    FILE* f = fopen(path.c_str(), "wb");
    CHECK(f && fwrite(p, 1, n, f) == n);
    fclose(f);
}

static void write_file(const std::string& path, int W, int H, int nh, int nv, int gop, int frames, bool flat)
{
    mdvt_video_writer* w = nullptr;
    CHECK((gop ? mdvt_video_create_stream(path.c_str(), W, H, 30, 1, nh, nv, 0, gop, &w) : mdvt_video_create(path.c_str(), W, H, 30, 1, nh, nv, &w)) == 0);
    for (int k = 0; k < frames; ++k) {
        const std::vector<uint8_t> f = frame_of(W, H, k, flat);
        CHECK(mdvt_video_write(w, f.data(), (size_t)W * 3, k & 1 ? MDVT_VIDEO_BGR : MDVT_VIDEO_RGB, 2) == 0);
    }
    int64_t n = 0;
    CHECK(mdvt_video_finish(w, &n) == 0 && n == frames);
}

static void round_trip(const std::string& dir, int W, int H, int nh, int nv, int gop)
{
    const std::string path = dir + "/rt.mkv";
    const int frames = 5;
    write_file(path, W, H, nh, nv, gop, frames, false);
    mdvt_video_reader* r = nullptr;
    mdvt_video_info info;
    CHECK(mdvt_video_open(path.c_str(), &r, &info) == 0);
    CHECK(info.width == W && info.height == H && info.frames == frames && info.coder_type == (gop ? 0 : 1));
    std::vector<uint8_t> got((size_t)(W * 3 + 5) * H);
    for (int k = 0; k < frames; ++k) {
        const std::vector<uint8_t> f = frame_of(W, H, k, false);
        CHECK(mdvt_video_read(r, got.data(), (size_t)W * 3 + 5, k & 1 ? MDVT_VIDEO_BGR : MDVT_VIDEO_RGB, 3) == 0);
        for (int y = 0; y < H; ++y) CHECK(memcmp(got.data() + (size_t)y * (W * 3 + 5), f.data() + (size_t)y * W * 3, (size_t)W * 3) == 0);
    }
    CHECK(mdvt_video_read(r, got.data(), (size_t)W * 3 + 5, MDVT_VIDEO_RGB, 0) == 1);
    CHECK(mdvt_video_seek(r, 4, 1) == 0 && mdvt_video_read(r, got.data(), (size_t)W * 3 + 5, MDVT_VIDEO_RGB, 1) == 0);
    mdvt_video_close(r);
    printf("round trip %dx%d slices %dx%d %s: ok\n", W, H, nh, nv, gop ? "stream writer" : "default writer");
}

static size_t find(const std::vector<uint8_t>& d, const char* pat, size_t n, size_t from = 0)
{
    const auto it = std::search(d.begin() + (ptrdiff_t)from, d.end(), pat, pat + n, [](uint8_t a, char b) { return a == (uint8_t)b; });
    CHECK(it != d.end());
    return (size_t)(it - d.begin());
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    const std::string dir = argv[1];
    for (int gop = 0; gop <= 3; gop += 3) {
        round_trip(dir, 1, 1, 0, 0, gop);
        round_trip(dir, 7, 5, 0, 0, gop);
        round_trip(dir, 33, 17, 4, 3, gop);
    }

    // two frames of 8x6 in one slice, flat: every element size around the patches is a one-byte EBML size
    const std::string good = dir + "/good.mkv", bad = dir + "/bad.mkv";
    write_file(good, 8, 6, 1, 1, 0, 2, true);
    const std::vector<uint8_t> file = slurp(good);
    mdvt_video_reader* r = nullptr;
    mdvt_video_info info;

    // (a) the TrackEntry ends one byte into the CodecID element's header: the child's data would begin past its parent's end
    {
        std::vector<uint8_t> d = file;
        const size_t tracks = find(d, "\x16\x54\xAE\x6B", 4);
        const size_t entry = tracks + 5;                              // Tracks: id, one-byte size; then the TrackEntry
        CHECK((d[tracks + 4] & 0x80) && d[entry] == 0xAE && (d[entry + 1] & 0x80));
        const size_t codec_id = find(d, "\x86\x86V_FFV1", 8, entry);
        const size_t size = codec_id + 1 - (entry + 2);
        CHECK(size < (size_t)(d[entry + 1] & 0x7F));
        d[entry + 1] = (uint8_t)(0x80 | size);
        spit(bad, d.data(), d.size());
        const int rc = mdvt_video_open(bad.c_str(), &r, &info);
        CHECK(rc < 0 && r == nullptr && strlen(mdvt_video_last_error()) > 0);
        printf("TrackEntry cut inside a child's header: %d, %s\n", rc, mdvt_video_last_error());
    }
    // (b) the file ends inside the first Cluster's SimpleBlock header: behind the element's id, before its size.  No frame is left,
    // and a file without frames is refused (as it was before for_children learnt to refuse (a))
    {
        const size_t cluster = find(file, "\x1F\x43\xB6\x75", 4);
        CHECK(file[cluster + 4] & 0x80);
        const size_t block = find(file, "\xE7\x81\x00\xA3", 4, cluster) + 3;
        CHECK(block == cluster + 8 && (file[block + 1] & 0x80));
        spit(bad, file.data(), block + 1);
        const int rc = mdvt_video_open(bad.c_str(), &r, &info);
        CHECK(rc == -3 && r == nullptr && strstr(mdvt_video_last_error(), "holds no video frames"));
        printf("file cut inside the first SimpleBlock's header: %d, %s\n", rc, mdvt_video_last_error());
    }
    return 0;
}
