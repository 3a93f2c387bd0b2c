// mdvt_matroska.h -- the container side of the host codec (mdvt_matroska.cpp): the reader's index of a Matroska file's one video
// track, and the writer's head, clusters and tail.  The two handles of the C ABI are defined here.  Internal.
#pragma once

#include "mdvt_ffv1_host.h"

namespace mdvt_host {

struct FileReader {
    FILE* fp = nullptr;
    uint64_t size = 0;
    ~FileReader() { if (fp) fclose(fp); }
    bool open(const char* path);
    bool read_at(uint64_t off, void* dst, size_t n);
};

struct FrameRef { uint64_t offset; uint32_t size; int64_t timecode; };

}  // namespace mdvt_host

struct mdvt_video_reader {
    mdvt_host::FileReader file;
    mdvt_host::Decoder dec;
    std::vector<mdvt_host::FrameRef> frames;
    size_t next = 0;
    std::vector<uint8_t> packet;
    std::vector<uint8_t> config;
    mdvt_video_info info{};
};

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
    std::vector<mdvt_host::GolombSliceState> golomb;
    ~mdvt_video_writer() { if (fp) fclose(fp); }
    uint64_t frame_ms(int64_t k) const { return (uint64_t)((k * 1000 * (int64_t)fps_den + fps_num / 2) / fps_num); }
};

namespace mdvt_host {

// the open file's video track: its frames in time order, its picture size and rate, and the FFV1 configuration record where the
// container holds one (parsed into r.dec and checked)
int index_matroska(mdvt_video_reader& r);

// The writer, one Cluster per frame.  write_head: the EBML header, the Segment's Info and Tracks (w's fields are set, w.fp is open);
// write_cluster: one packet, flagged and cued when `key`; write_tail: the Cues, then Duration and Segment size patched, w.fp closed
int write_head(mdvt_video_writer& w);
int write_cluster(mdvt_video_writer& w, const uint8_t* packet, size_t packet_size, bool key);
int write_tail(mdvt_video_writer& w);

}  // namespace mdvt_host
