"""TEST INFRASTRUCTURE: an independent planar (YCbCr) FFV1 encoder and decoder in plain Python, next to the RGB ones of
oracle/ffv1_ref.py and built from that module's primitives (range coder, Vlc, context_of, quant_tables, the Matroska muxer); the
oracle itself is imported, not edited.  RFC 9043 for colorspace_type 0, 8 bits, chroma_planes 1: a slice codes plane Y completely,
then Cb, then Cr; each plane line by line with 8-bit samples, no RCT, the run index restarting at each plane; Y uses the first
context set, Cb and Cr share the second.  A slice's chroma rectangle starts at (x0 >> hs, y0 >> vs) and is ceil(sw / 2^hs) x
ceil(sh / 2^vs).  Plus the colour conversion include/mdvt_video.h decrees, in NumPy, and the streams the CPU and GPU tests share.
Pure-Python loops: small frames only.  PARITY UNPINNED against FFmpeg's own yuv420p files (none can be made here)."""
import functools
import os
import struct
import tempfile

import numpy as np

from oracle import ffv1_ref as ref

PIX_FMTS = {"yuv444p": (0, 0), "yuv422p": (1, 0), "yuv420p": (1, 1)}


class Params(ref.Params):
    """ref.Params plus the fields a YCbCr record carries; anything FFV1 allows can be written (the refusals are tested with it)."""

    def __init__(self, pix_fmt="yuv420p", hs=None, vs=None, bits=8, colorspace=0, chroma_planes=1, **kw):
        super().__init__(**kw)
        self.hs, self.vs = PIX_FMTS[pix_fmt] if hs is None else (hs, vs)
        self.bits, self.colorspace, self.chroma_planes = bits, colorspace, chroma_planes


def _fields(rc, p, st):
    """The fields the configuration record and the version 0 / 1 frame header share, after `version` (and micro_version)."""
    rc.symbol(st, p.coder)
    assert p.coder != 2
    rc.symbol(st, p.colorspace)
    if p.version > 0:
        rc.symbol(st, p.bits)
    rc.put(st, 0, p.chroma_planes)
    rc.symbol(st, p.hs)
    rc.symbol(st, p.vs)
    rc.put(st, 0, p.alpha)


def config_record(p):
    rc = ref.RangeEncoder()
    st = [128] * 32
    rc.symbol(st, p.version)
    rc.symbol(st, p.micro)
    _fields(rc, p, st)
    rc.symbol(st, p.nh - 1)
    rc.symbol(st, p.nv - 1)
    rc.symbol(st, 1)
    for t in p.quant:
        ref.write_quant_table(rc, t)
    rc.put(st, 0, 0)
    rc.symbol(st, p.ec)
    rc.symbol(st, p.intra)
    rc.terminate(False)
    out = bytes(rc.out)
    return out + struct.pack(">I", ref.crc32_mpeg(out))


def chroma_rect(p, x0, y0, sw, sh):
    return x0 >> p.hs, y0 >> p.vs, -(-sw >> p.hs), -(-sh >> p.vs)


def chroma_shape(W, H, hs, vs):
    return -(-H >> vs), -(-W >> hs)


class _Slice:
    def __init__(self, p):
        self.p = p
        self.reset()

    def reset(self):
        n = self.p.context_count
        self.states = [[[128] * 32 for _ in range(n)] for _ in range(2)]
        self.vlc = [[ref.Vlc() for _ in range(n)] for _ in range(2)]


BITS = 8


def _encode_plane(p, states, vlcs, rc, bw, plane):
    h, w = plane.shape
    five, O = p.five(), 3
    last, cur = [0] * (w + 6), [0] * (w + 6)
    run_index = 0
    for y in range(h):
        last, cur = cur, last
        new = plane[y].tolist()
        cur[O - 1] = last[O]
        last[O + w] = last[O + w - 1]
        run_count = run_mode = 0
        for x in range(w):
            ctx = ref.context_of(p.quant, five, cur, last, O + x)
            L, LT, T = cur[O + x - 1], last[O + x - 1], last[O + x]
            diff = new[x] - ref.median(L, T, L + T - LT)
            cur[O + x] = new[x]
            if ctx < 0:
                ctx, diff = -ctx, -diff
            diff = ref.fold(diff, BITS)
            if p.coder:
                rc.symbol(states[ctx], diff, signed=True)
                continue
            if ctx == 0:
                run_mode = 1
            if run_mode:
                if diff:
                    while run_count >= 1 << ref.LOG2_RUN[run_index]:
                        run_count -= 1 << ref.LOG2_RUN[run_index]
                        run_index += 1
                        bw.put(1, 1)
                    bw.put(1 + ref.LOG2_RUN[run_index], run_count)
                    if run_index:
                        run_index -= 1
                    run_count = run_mode = 0
                    if diff > 0:
                        diff -= 1
                else:
                    run_count += 1
            if run_mode == 0:
                st = vlcs[ctx]
                v = ref.fold(diff - st.bias, BITS)
                k = st.k()
                code = v ^ ((2 * st.drift + st.count) >> 31)
                u = 2 * code if code >= 0 else -2 * code - 1
                if (u >> k) < 12:
                    bw.put((u >> k) + k + 1, (1 << k) + (u & ((1 << k) - 1)))
                else:
                    bw.put(12 + BITS, u - 11)
                st.update(v)
        if not p.coder and run_mode:
            while run_count >= 1 << ref.LOG2_RUN[run_index]:
                run_count -= 1 << ref.LOG2_RUN[run_index]
                run_index += 1
                bw.put(1, 1)
            if run_count:
                bw.put(1, 1)


def _get_vlc(br, st):
    k, q = st.k(), 0
    while q < 12 and not br.get1():
        q += 1
    u = ((q << k) | br.get(k)) if q < 12 else br.get(BITS) + 11
    v = (u >> 1) ^ -(u & 1)
    v ^= (2 * st.drift + st.count) >> 31
    ret = ref.fold(v + st.bias, BITS)
    st.update(v)
    return ret


def _decode_plane(p, states, vlcs, rd, br, h, w):
    five, O = p.five(), 3
    out = np.zeros((h, w), np.uint8)
    last, cur = [0] * (w + 6), [0] * (w + 6)
    run_index = 0
    for y in range(h):
        last, cur = cur, last
        cur[O - 1] = last[O]
        last[O + w] = last[O + w - 1]
        run_count = run_mode = 0
        for x in range(w):
            ctx = ref.context_of(p.quant, five, cur, last, O + x)
            sign = ctx < 0
            ctx = abs(ctx)
            if p.coder:
                d = rd.symbol(states[ctx], signed=True)
            else:
                if ctx == 0 and run_mode == 0:
                    run_mode = 1
                if run_mode:
                    if run_count == 0 and run_mode == 1:
                        if br.get1():
                            run_count = 1 << ref.LOG2_RUN[run_index]
                            if x + run_count <= w:
                                run_index += 1
                        else:
                            run_count = br.get(ref.LOG2_RUN[run_index])
                            if run_index:
                                run_index -= 1
                            run_mode = 2
                    run_count -= 1
                    if run_count < 0:
                        run_mode = run_count = 0
                        d = _get_vlc(br, vlcs[ctx])
                        if d >= 0:
                            d += 1
                    else:
                        d = 0
                else:
                    d = _get_vlc(br, vlcs[ctx])
            if sign:
                d = -d
            L, LT, T = cur[O + x - 1], last[O + x - 1], last[O + x]
            cur[O + x] = (ref.median(L, T, L + T - LT) + d) & ((1 << BITS) - 1)
        out[y] = cur[O:O + w]
    return out


def _slices(p, W, H):
    """[(luma rectangle, chroma rectangle)] of the frame's slices, in coding order"""
    if p.version < 3:
        return [((0, 0, W, H), chroma_rect(p, 0, 0, W, H))]
    out = []
    for i in range(p.nh * p.nv):
        r = ref.slice_rect(p, W, H, i % p.nh, i // p.nh)
        out.append((r, chroma_rect(p, *r)))
    return out


class Encoder:
    """(Y, Cb, Cr) uint8 planes -> FFV1 packets; a key frame every `gop` frames."""

    def __init__(self, p, W, H, gop=1):
        self.p, self.W, self.H, self.gop, self.n = p, W, H, gop, 0
        self.slices = [_Slice(p) for _ in _slices(p, W, H)]

    def encode(self, planes):
        p = self.p
        key = self.n % self.gop == 0
        self.n += 1
        packet = bytearray()
        for i, (sc, ((x0, y0, sw, sh), (cx0, cy0, cw, ch))) in enumerate(zip(self.slices, _slices(p, self.W, self.H))):
            rc = ref.RangeEncoder()
            if i == 0:
                rc.put([128], 0, 1 if key else 0)
                if key and p.version < 2:
                    st = [128] * 32
                    rc.symbol(st, p.version)
                    _fields(rc, p, st)
                    for t in p.quant:
                        ref.write_quant_table(rc, t)
            if p.version >= 3:
                st = [128] * 32
                for v in (i % p.nh, i // p.nh, 0, 0, 0, 0, 3, 0, 0):      # position, size - 1, two table indices, progressive, no aspect
                    rc.symbol(st, v)
            if key:
                sc.reset()
            sub = [planes[0][y0:y0 + sh, x0:x0 + sw], planes[1][cy0:cy0 + ch, cx0:cx0 + cw], planes[2][cy0:cy0 + ch, cx0:cx0 + cw]]
            assert sub[1].shape == (ch, cw) and sub[0].shape == (sh, sw)
            bw = None
            if not p.coder:
                rc.terminate(p.version > 2)
                bw = ref.BitWriter()
            for k, pl in enumerate(sub):
                _encode_plane(p, sc.states[min(k, 1)], sc.vlc[min(k, 1)], rc, bw, pl)
            if p.coder:
                rc.terminate(True)
                body = bytes(rc.out)
            else:
                body = bytes(rc.out) + bw.bytes()
            if p.version >= 3:
                body += struct.pack(">I", len(body))[1:]
                if p.ec:
                    body += b"\x00"
                    body += struct.pack(">I", ref.crc32_mpeg(body))
            packet += body
        return bytes(packet)


class Decoder:
    """Packets of a version 3 stream (range coder or Golomb-Rice, key and inter frames) -> (Y, Cb, Cr) planes."""

    def __init__(self, p, W, H):
        assert p.version == 3
        self.p, self.W, self.H = p, W, H
        self.slices = [_Slice(p) for _ in _slices(p, W, H)]

    def decode(self, packet):
        p = self.p
        ch, cw = chroma_shape(self.W, self.H, p.hs, p.vs)
        planes = [np.zeros((self.H, self.W), np.uint8), np.zeros((ch, cw), np.uint8), np.zeros((ch, cw), np.uint8)]
        n = p.nh * p.nv
        trailer = 3 + (5 if p.ec else 0)
        end, ext = len(packet), [None] * n
        for i in range(n - 1, -1, -1):
            size = int.from_bytes(packet[end - trailer:end - trailer + 3], "big")
            off = end - trailer - size
            assert off >= 0
            if p.ec:
                assert ref.crc32_mpeg(packet[off:end]) == 0, f"slice {i} CRC"
            ext[i] = (off, size)
            end = off
        assert end == 0
        rects = _slices(p, self.W, self.H)
        key = None
        for i, (off, size) in enumerate(ext):
            data = packet[off:off + size]
            rd = ref.RangeDecoder(data)
            if i == 0:
                key = rd.get([128], 0)
            st = [128] * 32
            sx, sy, w1, h1 = rd.symbol(st), rd.symbol(st), rd.symbol(st), rd.symbol(st)
            assert (w1, h1) == (0, 0) and rd.symbol(st) == 0 and rd.symbol(st) == 0
            rd.symbol(st), rd.symbol(st), rd.symbol(st)
            (x0, y0, sw, sh), (cx0, cy0, ccw, cch) = rects[sy * p.nh + sx]
            sc = self.slices[i]
            if key:
                sc.reset()
            br = None
            if not p.coder:
                rd.get([129], 0)
                br = ref.BitReader(data[rd.pos - 1:])
            planes[0][y0:y0 + sh, x0:x0 + sw] = _decode_plane(p, sc.states[0], sc.vlc[0], rd, br, sh, sw)
            planes[1][cy0:cy0 + cch, cx0:cx0 + ccw] = _decode_plane(p, sc.states[1], sc.vlc[1], rd, br, cch, ccw)
            planes[2][cy0:cy0 + cch, cx0:cx0 + ccw] = _decode_plane(p, sc.states[1], sc.vlc[1], rd, br, cch, ccw)
        return planes


# ------------------------------------------------------------------------------------------------------------ the conversion
def convert(planes, hs, vs, bgr=False):
    """include/mdvt_video.h's decree, written from its text: chroma replicated; c = Y - 16, d = U - 128, e = V - 128;
    R = clip8((298 c + 409 e + 128) >> 8), G = clip8((298 c - 100 d - 208 e + 128) >> 8), B = clip8((298 c + 516 d + 128) >> 8)."""
    Y, Cb, Cr = (np.asarray(a) for a in planes)
    H, W = Y.shape
    yy, xx = np.mgrid[0:H, 0:W]
    c = Y.astype(np.int32) - 16
    d = Cb[yy >> vs, xx >> hs].astype(np.int32) - 128
    e = Cr[yy >> vs, xx >> hs].astype(np.int32) - 128
    r = np.clip((298 * c + 409 * e + 128) >> 8, 0, 255)
    g = np.clip((298 * c - 100 * d - 208 * e + 128) >> 8, 0, 255)
    b = np.clip((298 * c + 516 * d + 128) >> 8, 0, 255)
    return np.stack([b, g, r] if bgr else [r, g, b], -1).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------ shared streams
def planes_content(N, H, W, hs, vs, seed):
    """Frame t: luma flat with a ramp in the middle third and noise bands on the right (runs of every length, runs cut by the
    row's end, escapes); chroma flat, a ramp and noise in one corner; both pass below 16 and above 240, so the conversion clips."""
    rng = np.random.default_rng(seed)
    ch, cw = chroma_shape(W, H, hs, vs)
    out = []
    for t in range(N):
        y, x = np.mgrid[0:H, 0:W]
        Y = np.full((H, W), (40 + 3 * t) % 256, np.uint8)
        mid = (x >= W // 3) & (x < W - W // 3)
        Y[mid] = (((x + y + t) * 5) % 256)[mid]
        noisy = (x > W // 2) & ((y // 4 + t) % 3 == 0)
        Y[noisy] = rng.integers(0, 256, int(noisy.sum()), dtype=np.uint8)
        Y[max(0, H - 2):] = 250
        y, x = np.mgrid[0:ch, 0:cw]
        Cb = np.full((ch, cw), (128 + 7 * t) % 256, np.uint8)
        Cr = ((x * 9 + y * 3 + 11 * t) % 256).astype(np.uint8)
        Cr[:, :cw // 2] = 90
        corner = (x >= cw - max(1, cw // 3)) & (y < max(1, ch // 2))
        Cb[corner] = rng.integers(0, 256, int(corner.sum()), dtype=np.uint8)
        out.append((Y, Cb, Cr))
    return out


# (W, H, frames, pix_fmt, coder, ec, gop, intra, (nh, nv), version)
def _matrix():
    m = []
    for pix in PIX_FMTS:
        for coder in (0, 1):
            for intra, gop in ((1, 1), (0, 3)):
                for ec in (0, 1):
                    m.append((34, 22, 7, pix, coder, ec, gop, intra, (1, 1), 3))      # odd chroma width and height
                m.append((34, 22, 7, pix, coder, 0, gop, 0, (1, 1), 1))
            m.append((33, 21, 7, pix, coder, 1, 3, 0, (1, 1), 3))          # odd luma: ceil on both chroma axes
            m.append((64, 48, 7, pix, coder, 1, 3, 0, (2, 2), 3))
    for coder in (0, 1):                                               # slice origins at x = 16, y = 10: odd slice sizes, aligned origins
        m.append((33, 21, 7, "yuv420p", coder, 1, 3, 0, (2, 2), 3))
    return m


MATRIX = _matrix()
MATRIX_V3 = [c for c in MATRIX if c[9] == 3]


def case_id(c):
    W, H, N, pix, coder, ec, gop, intra, (nh, nv), version = c
    return f"{W}x{H}x{N}-{pix}-coder{coder}-ec{ec}-gop{gop}-intra{intra}-{nh}x{nv}-v{version}"


def params_of(case):
    W, H, N, pix, coder, ec, gop, intra, (nh, nv), version = case
    return Params(pix_fmt=pix, version=version, coder=coder, ec=ec, intra=intra, nh=nh, nv=nv)


@functools.lru_cache(maxsize=None)
def make_stream(case, seed=31):
    """-> (planes per frame, convert(planes) as N x H x W x 3 RGB, packets, configuration record (empty for version 1))"""
    W, H, N, pix, coder, ec, gop, intra, sl, version = case
    p = params_of(case)
    planes = planes_content(N, H, W, p.hs, p.vs, seed)
    enc = Encoder(p, W, H, gop=gop)
    packets = tuple(enc.encode(pl) for pl in planes)
    rgb = np.stack([convert(pl, p.hs, p.vs) for pl in planes])
    return planes, rgb, packets, (config_record(p) if version >= 3 else b"")


def mux(packets, W, H, cfg):
    return ref.mux_matroska(list(packets), W, H, 30, cfg)


def host_read(packets, cfg, W, H, bgr=False):
    """The host reader on a Matroska file of the packets -> (frames, pix_fmt)"""
    from metric_depth_video_toolbox_amd import video_io
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "y.mkv")
        with open(path, "wb") as f:
            f.write(mux(packets, W, H, cfg))
        with video_io.VideoReader(path, bgr=bgr, threads=1) as r:
            return np.stack(list(r)), r.pix_fmt


def host_stream_decode(packets, cfg, W, H, bgr=False):
    """The packet-to-packet host decoder (the device's arbiter) -> frames"""
    from metric_depth_video_toolbox_amd import video_io
    with video_io.StreamDecoder(cfg, W, H, bgr=bgr) as d:
        return np.stack([d.decode(p) for p in packets])


# ------------------------------------------------------------------------------------------------------------ damaged packets
def damage_variants():
    """tests/ffv1_streams.py's scheme on a YCbCr key frame: one small Golomb-Rice yuv420p frame in 2 x 2 slices without CRCs, so
    that whatever is in it reaches the decoder: every single-bit flip, every truncation, and seeded random corruptions.
    -> W, H, configuration record, the intact frame (RGB), variants"""
    W, H, nh, nv = 20, 12, 2, 2
    p = Params(pix_fmt="yuv420p", coder=0, ec=0, intra=0, nh=nh, nv=nv)
    planes = planes_content(1, H, W, p.hs, p.vs, 5)[0]
    cfg, pkt = config_record(p), Encoder(p, W, H, gop=4).encode(planes)
    variants = [pkt]
    for i in range(len(pkt) * 8):
        b = bytearray(pkt); b[i >> 3] ^= 0x80 >> (i & 7); variants.append(bytes(b))
    variants += [pkt[:k] for k in range(len(pkt))]
    rng = np.random.default_rng(20261019)
    for k in range(300):
        b = bytearray(pkt)
        if k % 3 == 0:
            for _ in range(2 + k % 5):
                b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        elif k % 3 == 1:
            cut = int(rng.integers(0, len(b)))
            b = b[:cut] + bytearray(rng.integers(0, 256, len(pkt) - cut, dtype=np.uint8).tobytes())
        else:                                                          # the payload damaged, the slice sizes intact
            i = int(rng.integers(0, max(1, len(b) - 3 * nh * nv)))
            b[i:i + 4] = rng.integers(0, 256, len(b[i:i + 4]), dtype=np.uint8).tobytes()
        variants.append(bytes(b))
    return W, H, cfg, convert(planes, p.hs, p.vs), variants


# (index into damage_variants()'s variants, the core's status word): a fixed handful for the GPU, which needs no compiler for them;
# tests/test_ffv1_ycbcr_cpu.py asserts that the host program gives exactly these
DAMAGED_PICKS = ((0, 0), (17, 0), (140, 0), (333, 0), (700, 0), (2512, 0), (2514, 0), (1, 5), (265, 5), (2216, 5), (2, 2), (5, 2))


# ------------------------------------------------------------------------------------------------------------ the host program
_programs = {}


def build_host_program(sanitize):
    """tests/ffv1_ycbcr_decode_host.cpp, built the way ffv1_streams.build_host_program builds its program -> (path, None) or (None, why)"""
    import shutil
    import subprocess
    import ffv1_streams as fs
    if sanitize in _programs:
        return _programs[sanitize]
    gxx = shutil.which("g++")
    if not gxx:
        _programs[sanitize] = (None, "no g++")
        return _programs[sanitize]
    tmp = tempfile.mkdtemp(prefix="ffv1_ycbcr_core_")
    exe = os.path.join(tmp, "ffv1_ycbcr_decode_host_asan" if sanitize else "ffv1_ycbcr_decode_host")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", fs.CSRC, "-o", exe, os.path.join(fs.REPO, "tests", "ffv1_ycbcr_decode_host.cpp")]
    if sanitize:
        cmd[3:3] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    no_runtime = any(t in r.stderr for t in ("cannot find -lasan", "cannot find -lubsan", "libasan.a", "libubsan.a", "unrecognized"))
    if r.returncode and sanitize and no_runtime:
        _programs[sanitize] = (None, r.stderr[-400:])
    else:
        assert r.returncode == 0, r.stderr[-3000:]
        _programs[sanitize] = (exe, None)
    return _programs[sanitize]
