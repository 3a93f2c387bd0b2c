// mdvt_video.cpp -- the C ABI of include/mdvt_video.h and include/mdvt_video_stream.h (libmdvt_video.so): FFV1 (RFC 9043) in
// Matroska (RFC 9559 / EBML RFC 8794), reader and writer.
//
// Host C++17, no third-party library.  What the reference does with OpenCV's FFmpeg back end -- cv2.VideoCapture over the
// toolbox's *_depth.mkv files (stereo_rerender.py:326-341) and cv2.VideoWriter(fourcc 'FFV1') for the stereo / infill-mask /
// depth outputs (stereo_rerender.py:426-444, 941; depth_frames_helper.py:125-161) -- written from the specifications, in parts:
//   mdvt_ffv1_dec.cpp   the FFV1 decoder            mdvt_matroska.cpp   the container, read and written
//   mdvt_ffv1_enc.cpp   the FFV1 encoders           csrc/mdvt_ffv1_core.h   the FFV1 primitives, shared with the device
// This file holds the entry points alone: argument checks and calls into those parts, each body inside the exception barrier.
#include "mdvt_matroska.h"

#include <memory>

using namespace mdvt_host;

struct mdvt_ffv1_stream_decoder { Decoder dec; };

namespace {

void fill_codec_info(mdvt_video_reader& r)
{
    const Ffv1Config& f = r.dec.f;
    r.info.ffv1_version = f.version; r.info.ffv1_micro_version = f.micro; r.info.coder_type = f.coder;
    r.info.slices = f.version >= 3 ? f.nh * f.nv : 1; r.info.alpha = f.alpha; r.info.intra = f.intra; r.info.ec = f.ec;
    r.info.pix_fmt = f.pix_fmt();
}

int read_frame(mdvt_video_reader* r, uint8_t* dst, size_t pitch, int order, int threads)
{
    if (r->next >= r->frames.size()) return 1;
    const FrameRef& fr = r->frames[r->next];
    r->packet.resize(fr.size);
    if (!r->file.read_at(fr.offset, r->packet.data(), fr.size)) return fail(ERR_IO, "short read of frame %zu", r->next);
    const int rc = r->dec.decode_frame(r->packet.data(), r->packet.size(), dst, pitch, order, threads);
    if (rc) return rc;
    ++r->next;
    return 0;
}

// the key-frame bit of frame k's packet, or -1
int packet_is_key(mdvt_video_reader* r, size_t k)
{
    uint8_t b[2];
    if (r->frames[k].size < 2 || !r->file.read_at(r->frames[k].offset, b, 2)) return -1;
    return key_frame_bit(b[0], b[1]);
}

int create_writer(const char* path, int width, int height, int fps_num, int fps_den, int slices_h, int slices_v, int coder, int gop,
                  mdvt_video_writer** out)
{
    if (!path || !out || width < 1 || height < 1 || fps_num < 1 || fps_den < 1) return fail(ERR_ARG, "bad argument");
    if (slices_h == 0 && slices_v == 0) { slices_h = std::min(4, width); slices_v = std::min(4, height); }
    if (slices_h < 1 || slices_v < 1 || slices_h > width || slices_v > height || slices_h * slices_v > 1024) return fail(ERR_ARG, "bad slice counts");
    *out = nullptr;
    std::unique_ptr<mdvt_video_writer> w(new mdvt_video_writer());
    w->fp = fopen(path, "wb");
    if (!w->fp) return fail(ERR_IO, "cannot create %s", path);
    w->W = width; w->H = height; w->nh = slices_h; w->nv = slices_v; w->fps_num = fps_num; w->fps_den = fps_den;
    w->coder = coder; w->gop = gop;
    const int rc = write_head(*w);
    if (rc) return rc;
    *out = w.release();
    return 0;
}

int write_packet(mdvt_video_writer* w, const uint8_t* packet, size_t packet_size)
{
    if (!w || !packet || packet_size < 8) return fail(ERR_ARG, "bad argument");
    return write_cluster(*w, packet, packet_size, key_frame_bit(packet[0], packet[1]) != 0);       // the packet's first range-coded bit
}

}  // namespace

extern "C" {

const char* mdvt_video_last_error(void) { return g_err.c_str(); }      // (these two have nothing that throws)
int mdvt_video_abi(void) { return MDVT_VIDEO_ABI; }

int mdvt_video_open(const char* path, mdvt_video_reader** out, mdvt_video_info* info)
{
    return guarded([&]() {
        if (!path || !out) return fail(ERR_ARG, "NULL argument");
        *out = nullptr;
        std::unique_ptr<mdvt_video_reader> r(new mdvt_video_reader());
        if (!r->file.open(path)) return fail(ERR_IO, "cannot open %s", path);
        int rc = index_matroska(*r);
        if (rc) return rc;
        if (r->frames.empty()) return fail(ERR_FORMAT, "%s holds no video frames", path);
        if (!r->dec.have_config) {
            // versions 0 / 1: the parameters are inside the first key frame -- decode it once into a scratch picture to learn them
            std::vector<uint8_t> scratch((size_t)r->info.width * 3 * (size_t)r->info.height);
            rc = read_frame(r.get(), scratch.data(), (size_t)r->info.width * 3, MDVT_VIDEO_RGB, 0);
            if (rc < 0) return rc;
            r->next = 0;
            r->dec.key_frame_ok = false;
        }
        fill_codec_info(*r);
        if (info) *info = r->info;
        *out = r.release();
        return 0;
    });
}

int mdvt_video_read(mdvt_video_reader* r, uint8_t* dst, size_t pitch, int order, int threads)
{
    return guarded([&]() {
        if (!r || !dst) return fail(ERR_ARG, "NULL argument");
        if (pitch < (size_t)r->info.width * 3) return fail(ERR_ARG, "pitch smaller than one row");
        if (order != MDVT_VIDEO_RGB && order != MDVT_VIDEO_BGR) return fail(ERR_ARG, "order must be MDVT_VIDEO_RGB or MDVT_VIDEO_BGR");
        return read_frame(r, dst, pitch, order, threads);
    });
}

int mdvt_video_rewind(mdvt_video_reader* r)
{
    return guarded([&]() {
        if (!r) return fail(ERR_ARG, "NULL argument");
        r->next = 0;
        r->dec.key_frame_ok = false;
        return 0;
    });
}

int mdvt_video_seek(mdvt_video_reader* r, int64_t frame, int threads)
{
    return guarded([&]() {
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
            const int rc = read_frame(r, scratch.data(), (size_t)r->info.width * 3, MDVT_VIDEO_RGB, threads);
            if (rc) return rc < 0 ? rc : fail(ERR_DATA, "unexpected end of the video");
        }
        return 0;
    });
}

int mdvt_video_next_packet(mdvt_video_reader* r, uint8_t* packet, size_t packet_cap, size_t* packet_size)
{
    return guarded([&]() {
        if (!r || !packet || !packet_size) return fail(ERR_ARG, "NULL argument");
        if (r->next >= r->frames.size()) return 1;
        const FrameRef& fr = r->frames[r->next];
        if (fr.size > packet_cap) return fail(ERR_ARG, "packet buffer too small: %u needed", fr.size);
        if (!r->file.read_at(fr.offset, packet, fr.size)) return fail(ERR_IO, "short read of frame %zu", r->next);
        *packet_size = fr.size;
        ++r->next;
        r->dec.key_frame_ok = false;          // the decoder did not see this frame: the next decode must start at a key frame
        return 0;
    });
}

int mdvt_video_config_record(mdvt_video_reader* r, uint8_t* config, size_t config_cap, size_t* config_size)
{
    return guarded([&]() {
        if (!r || !config_size) return fail(ERR_ARG, "NULL argument");
        if (r->config.size() > config_cap || (!config && !r->config.empty())) return fail(ERR_ARG, "config buffer too small: %zu needed", r->config.size());
        if (!r->config.empty()) memcpy(config, r->config.data(), r->config.size());
        *config_size = r->config.size();
        return 0;
    });
}

void mdvt_video_close(mdvt_video_reader* r) { (void)guarded([&]() { delete r; return 0; }); }

int mdvt_ffv1_encode_frame(int width, int height, int slices_h, int slices_v, const uint8_t* src, size_t pitch, int order, int threads,
                           uint8_t* packet, size_t packet_cap, size_t* packet_size, uint8_t* config, size_t config_cap, size_t* config_size)
{
    return guarded([&]() {
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
    });
}

int mdvt_ffv1_decode_frame(int width, int height, const uint8_t* config, size_t config_size, const uint8_t* packet, size_t packet_size,
                           uint8_t* dst, size_t pitch, int order, int threads)
{
    return guarded([&]() {
        if (!config || !packet || !dst || width < 1 || height < 1 || pitch < (size_t)width * 3) return fail(ERR_ARG, "bad argument");
        Decoder dec;
        dec.W = width; dec.H = height;
        int rc = parse_config_record(config, config_size, dec.f);
        if (rc) return rc;
        dec.have_config = true;
        rc = dec.check_supported();
        if (rc) return rc;
        return dec.decode_frame(packet, packet_size, dst, pitch, order, threads);
    });
}

int mdvt_video_create(const char* path, int width, int height, int fps_num, int fps_den, int slices_h, int slices_v, mdvt_video_writer** out)
{
    return guarded([&]() { return create_writer(path, width, height, fps_num, fps_den, slices_h, slices_v, 1, 1, out); });
}

int mdvt_video_create_stream(const char* path, int width, int height, int fps_num, int fps_den, int slices_h, int slices_v, int coder_type,
                             int gop, mdvt_video_writer** out)
{
    return guarded([&]() {
        if (coder_type != 0) return fail(ERR_ARG, "coder_type %d: the stream class is Golomb-Rice (0); mdvt_video_create writes the range coder's", coder_type);
        if (gop < 1) return fail(ERR_ARG, "gop must be >= 1");
        return create_writer(path, width, height, fps_num, fps_den, slices_h, slices_v, 0, gop, out);
    });
}

int mdvt_video_write(mdvt_video_writer* w, const uint8_t* src, size_t pitch, int order, int threads)
{
    return guarded([&]() {
        if (!w || !src) return fail(ERR_ARG, "NULL argument");
        if (pitch < (size_t)w->W * 3) return fail(ERR_ARG, "pitch smaller than one row");
        if (order != MDVT_VIDEO_RGB && order != MDVT_VIDEO_BGR) return fail(ERR_ARG, "order must be MDVT_VIDEO_RGB or MDVT_VIDEO_BGR");
        int rc = w->coder ? encode_frame(w->W, w->H, w->nh, w->nv, src, pitch, order, threads, w->packet)
                          : encode_frame_golomb(w->W, w->H, w->nh, w->nv, src, pitch, order, threads, w->frames % w->gop == 0, w->golomb, w->packet);
        if (rc) return rc;
        return write_packet(w, w->packet.data(), w->packet.size());
    });
}

int mdvt_video_write_packet(mdvt_video_writer* w, const uint8_t* packet, size_t packet_size)
{
    return guarded([&]() { return write_packet(w, packet, packet_size); });
}

int mdvt_video_seek_packet(mdvt_video_reader* r, int64_t frame)
{
    return guarded([&]() {
        if (!r) return fail(ERR_ARG, "NULL argument");
        if (frame < 0 || frame > (int64_t)r->frames.size()) return fail(ERR_ARG, "frame %lld outside 0..%zu", (long long)frame, r->frames.size());
        r->next = (size_t)frame;
        r->dec.key_frame_ok = false;          // nothing is decoded on the way: the next decode must start at a key frame
        return 0;
    });
}

int mdvt_video_packet_is_key(mdvt_video_reader* r, int64_t frame)
{
    return guarded([&]() {
        if (!r) return fail(ERR_ARG, "NULL argument");
        if (frame < 0 || frame >= (int64_t)r->frames.size()) return fail(ERR_ARG, "frame %lld outside 0..%zu", (long long)frame, r->frames.size());
        const int key = packet_is_key(r, (size_t)frame);
        return key < 0 ? fail(ERR_IO, "short read of frame %lld", (long long)frame) : key;
    });
}

int mdvt_ffv1_stream_decoder_create(int width, int height, const uint8_t* config, size_t config_size, mdvt_ffv1_stream_decoder** out)
{
    return guarded([&]() {
        if (!config || !out || width < 1 || height < 1) return fail(ERR_ARG, "bad argument");
        *out = nullptr;
        std::unique_ptr<mdvt_ffv1_stream_decoder> d(new mdvt_ffv1_stream_decoder());
        d->dec.W = width; d->dec.H = height;
        int rc = parse_config_record(config, config_size, d->dec.f);
        if (!rc) { d->dec.have_config = true; rc = d->dec.check_supported(); }
        if (rc) return rc;
        *out = d.release();
        return 0;
    });
}

int mdvt_ffv1_stream_decoder_decode(mdvt_ffv1_stream_decoder* d, const uint8_t* packet, size_t packet_size, uint8_t* dst, size_t pitch, int order,
                                    int threads)
{
    return guarded([&]() {
        if (!d || !packet || !dst || pitch < (size_t)d->dec.W * 3) return fail(ERR_ARG, "bad argument");
        if (order != MDVT_VIDEO_RGB && order != MDVT_VIDEO_BGR) return fail(ERR_ARG, "order must be MDVT_VIDEO_RGB or MDVT_VIDEO_BGR");
        return d->dec.decode_frame(packet, packet_size, dst, pitch, order, threads);
    });
}

void mdvt_ffv1_stream_decoder_destroy(mdvt_ffv1_stream_decoder* d) { (void)guarded([&]() { delete d; return 0; }); }

int mdvt_video_finish(mdvt_video_writer* w, int64_t* frames)
{
    return guarded([&]() {
        if (!w) return fail(ERR_ARG, "NULL argument");
        std::unique_ptr<mdvt_video_writer> own(w);
        const int rc = write_tail(*w);
        if (frames) *frames = w->frames;
        return rc;
    });
}

}  // extern "C"
