// mdvt_matroska.cpp -- Matroska (RFC 9559 / EBML RFC 8794) around the FFV1 packets: one video track, CodecID V_FFV1 with the
// configuration record as CodecPrivate (reader also: V_MS/VFW/FOURCC with a BITMAPINFOHEADER 'FFV1' followed by the record, or
// nothing for versions 0 / 1), SimpleBlocks (reader also: BlockGroups) in Clusters, Cues at the end, Duration and Segment size
// patched on finish.
#include "mdvt_matroska.h"

#include <stdlib.h>

#include <functional>

namespace mdvt_host {

namespace {

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

}  // namespace

bool FileReader::open(const char* path)
{
    fp = fopen(path, "rb");
    if (!fp) return false;
    fseeko(fp, 0, SEEK_END);
    size = (uint64_t)ftello(fp);
    fseeko(fp, 0, SEEK_SET);
    return true;
}

bool FileReader::read_at(uint64_t off, void* dst, size_t n) { return fseeko(fp, (off_t)off, SEEK_SET) == 0 && fread(dst, 1, n, fp) == n; }

namespace {

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

// walks the children of a master element [off, end); false where the structure is damaged
template <class F>
bool for_children(FileReader& f, uint64_t off, uint64_t end, F&& fn)
{
    while (off < end) {
        uint32_t id; uint64_t size;
        const int h = read_element_header(f, off, &id, &size);             // (read against the file's size, not the parent's end)
        if (!h) return false;
        uint64_t data = off + (uint64_t)h;
        if (data > end) return false;                         // the child's header straddles its parent's end
        if (size == kUnknownSize) size = end - data;          // (only Segment / Cluster may be unknown-sized: runs to the parent's end)
        if (data + size > end) size = end - data;             // a truncated file: take what is there
        if (!fn(id, data, size)) return false;
        off = data + size;
    }
    return true;
}

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

// ---- writer ----
int write_head(mdvt_video_writer& w)
{
    EbmlBuf head, eb;
    eb.uint_el(ID_EBMLVERSION, 1); eb.uint_el(ID_EBMLREADVERSION, 1); eb.uint_el(ID_EBMLMAXIDLENGTH, 4); eb.uint_el(ID_EBMLMAXSIZELENGTH, 8);
    eb.str_el(ID_DOCTYPE, "matroska"); eb.uint_el(ID_DOCTYPEVERSION, 4); eb.uint_el(ID_DOCTYPEREADVERSION, 2);
    head.master(ID_EBML, eb);
    head.id(ID_SEGMENT);
    w.segment_size_pos = head.b.size();
    head.size_n(0, 8);                                   // patched by write_tail
    w.segment_data = head.b.size();
    EbmlBuf info;
    info.uint_el(ID_TIMECODESCALE, 1000000);
    info.str_el(ID_MUXINGAPP, "mdvt_video");
    info.str_el(ID_WRITINGAPP, "metric_depth_video_toolbox_amd");
    info.id(ID_DURATION); info.size(8);
    const size_t dur_in_info = info.b.size();
    for (int k = 0; k < 8; ++k) info.b.push_back(0);
    head.id(ID_INFO); head.size(info.b.size());
    w.duration_pos = head.b.size() + dur_in_info;
    head.b.insert(head.b.end(), info.b.begin(), info.b.end());
    EbmlBuf video, entry, tracks;
    video.uint_el(ID_PIXELWIDTH, (uint64_t)w.W); video.uint_el(ID_PIXELHEIGHT, (uint64_t)w.H);
    entry.uint_el(ID_TRACKNUMBER, 1); entry.uint_el(ID_TRACKUID, 1); entry.uint_el(ID_TRACKTYPE, 1); entry.uint_el(ID_FLAGLACING, 0);
    entry.uint_el(ID_DEFAULTDURATION, (uint64_t)((1000000000.0 * w.fps_den) / w.fps_num + 0.5));
    entry.str_el(ID_CODECID, "V_FFV1");
    const std::vector<uint8_t> rec = make_config_record(w.nh, w.nv, w.coder, w.coder ? 1 : 0);
    entry.bin_el(ID_CODECPRIVATE, rec.data(), rec.size());
    entry.master(ID_VIDEO, video);
    tracks.master(ID_TRACKENTRY, entry);
    head.master(ID_TRACKS, tracks);
    if (fwrite(head.b.data(), 1, head.b.size(), w.fp) != head.b.size()) return fail(ERR_IO, "write failed");
    return 0;
}

// one Cluster per frame; a key frame (every frame of the default, intra-only class) is flagged in its block and gets a cue: a seek
// point.  An inter frame of the stream class is neither.
int write_cluster(mdvt_video_writer& w, const uint8_t* packet, size_t packet_size, bool key)
{
    const uint64_t tc = w.frame_ms(w.frames);
    EbmlBuf cl, body;
    body.uint_el(ID_TIMECODE, tc);
    body.id(ID_SIMPLEBLOCK); body.size(packet_size + 4);
    body.b.push_back(0x81); body.b.push_back(0); body.b.push_back(0); body.b.push_back(key ? 0x80 : 0x00);   // track 1, relative time 0, key frame
    cl.id(ID_CLUSTER); cl.size(body.b.size() + packet_size);
    const uint64_t pos = (uint64_t)ftello(w.fp);
    if (fwrite(cl.b.data(), 1, cl.b.size(), w.fp) != cl.b.size() || fwrite(body.b.data(), 1, body.b.size(), w.fp) != body.b.size() ||
        fwrite(packet, 1, packet_size, w.fp) != packet_size)
        return fail(ERR_IO, "write failed (disk full?)");
    if (key) w.cues.push_back({tc, pos - w.segment_data});
    ++w.frames;
    return 0;
}

int write_tail(mdvt_video_writer& w)
{
    int rc = 0;
    EbmlBuf cues;
    for (auto& c : w.cues) {
        EbmlBuf pos, pt;
        pos.uint_el(ID_CUETRACK, 1); pos.uint_el(ID_CUECLUSTERPOSITION, c.second);
        pt.uint_el(ID_CUETIME, c.first); pt.master(ID_CUETRACKPOSITIONS, pos);
        cues.master(ID_CUEPOINT, pt);
    }
    EbmlBuf tail;
    tail.master(ID_CUES, cues);
    if (fwrite(tail.b.data(), 1, tail.b.size(), w.fp) != tail.b.size()) rc = fail(ERR_IO, "write failed");
    const uint64_t end = (uint64_t)ftello(w.fp);
    EbmlBuf sz;
    sz.size_n(end - w.segment_data, 8);
    uint8_t dur[8];
    const double d = (double)w.frame_ms(w.frames);
    uint64_t u;
    memcpy(&u, &d, 8);
    for (int k = 0; k < 8; ++k) dur[k] = (uint8_t)(u >> (8 * (7 - k)));
    if (fseeko(w.fp, (off_t)w.segment_size_pos, SEEK_SET) || fwrite(sz.b.data(), 1, 8, w.fp) != 8 ||
        fseeko(w.fp, (off_t)w.duration_pos, SEEK_SET) || fwrite(dur, 1, 8, w.fp) != 8)
        rc = fail(ERR_IO, "patching the headers failed");
    FILE* fp = w.fp;
    w.fp = nullptr;
    if (fclose(fp)) rc = fail(ERR_IO, "close failed");
    return rc;
}

}  // namespace mdvt_host
