"""mdvt_decode_video_frames (include/mdvt_ffv1_decode.h) held to its footprint with the arenas of tests/footprint.py, through the
raw C ABI: exactly the first 3 * width bytes of each row of each frame, n_frames status words, nothing else; every byte inside is
written; the result does not depend on the bytes behind a packet's end; a refused call leaves everything as it was.  (The entry point
is declared outside include/mdvt.h, so its case family lives here and not in test_gpu_footprint.py; its tally row is printed here
and taken out of the shared table again.)"""
import ctypes as C

import numpy as np
import pytest

import footprint as fp

pytestmark = pytest.mark.gpu

ENTRY = "mdvt_decode_video_frames"
UNSUPPORTED, INVALID = -3, -1


def _vp(a):
    return C.c_void_p(a.ptr)


@pytest.fixture()
def own_tally():
    try:
        yield
    finally:
        fp.TALLY.pop(ENTRY, None)                      # test_gpu_footprint.py's table lists include/mdvt.h's entry points only


def test_decode_video_frames_footprint(own_tally):
    import torch
    from metric_depth_video_toolbox_amd import _lib, video_io
    from oracle import ffv1_ref as ref
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    try:
        for k, (rng, lays) in enumerate(fp.layout_sweep(10, 560)):
            W = int(rng.choice(fp.WIDTHS[:20]))
            H = int(rng.choice(fp.HEIGHTS))
            N = 1 + k % 3
            order = k % 2
            slices = (min((1, 2, 3, 4)[k % 4], W), min((1, 2, 5)[k % 3], H))
            frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
            frames[0, :, : W // 2] = 40
            if k % 5 == 4:                             # packets without CRCs: the independent encoder
                p = ref.Params(nh=slices[0], nv=slices[1], ec=0)
                enc = ref.StreamEncoder(p, W, H)
                packets, cfg = [enc.encode(f) for f in frames], ref.config_record(p)
            else:
                pk = [video_io.encode_frame(f, slices=slices) for f in frames]
                packets, cfg = [x[0] for x in pk], pk[0][1]
            tail = int(rng.integers(0, 9))             # bytes behind every packet: part of the blob, not of a packet -- they hold poison
            sizes = np.array([len(x) for x in packets], np.uint32)
            offs = np.zeros(N, np.uint64)
            total = 0
            for f in range(N):
                offs[f] = total
                total += len(packets[f]) + tail
            ld, lb, lst = lays.u8(), lays.u8(), fp.Layout(int(rng.choice(fp.BASES4)))
            loff = fp.Layout(int(rng.choice((0, 8))))

            def body(run, bad_cfg=None, short=False):
                blob = run.out("blob", 1, total, 1, fp.Layout(lb.base, 0, 0))      # poison between the packets ...
                host = blob.read()
                for f in range(N):
                    host[blob.start + int(offs[f]): blob.start + int(offs[f]) + len(packets[f])] = np.frombuffer(packets[f], np.uint8)
                blob.buf.copy_(torch.from_numpy(host))
                blob.input = host[blob.start: blob.start + total].reshape(1, 1, total).copy()      # ... and an input all the same
                o = run.inp("offsets", offs.view(np.uint8).reshape(1, 1, -1), loff)
                s = run.inp("sizes", sizes.view(np.uint8).reshape(1, 1, -1), lst)
                d = run.out("dst", H, 3 * W, N, ld)
                st = run.out("status", 1, 4 * N, 1, lst)
                c = bad_cfg if bad_cfg is not None else cfg
                rc = L.mdvt_decode_video_frames(ctx.handle, W, H, c, len(c), _vp(blob), total, _vp(o), _vp(s), N, _vp(d),
                                                3 * W - 1 if short else d.pitch, d.stride, order, _vp(st), None)
                if bad_cfg is None and not short:
                    ctx.check(rc)
                return rc
            tag = f"{W}x{H} x{N} slices={slices} order={order} tail={tail} {ld} {lb}"
            out = fp.twice(ENTRY, body, seed=k, what=tag)
            fp.accepted(ENTRY)
            assert not np.ascontiguousarray(out["status"]).view(np.uint32).any(), tag
            want = frames[..., ::-1] if order else frames
            assert np.array_equal(out["dst"].reshape(N, H, W, 3), want), tag
            if k % 4 == 0:
                fp.refused(ENTRY, lambda run: body(run, short=True), INVALID, seed=k)
                golomb = ref.config_record(ref.Params(coder=0, nh=slices[0], nv=slices[1]))
                fp.refused(ENTRY, lambda run: body(run, bad_cfg=golomb), UNSUPPORTED, seed=k)
        fp.finish_entry(ENTRY)
        t = fp.tally(ENTRY)
        assert t["refused"] >= 4 and t["outside_bytes"] >= 2 * 4096 * t["accepted"]
    finally:
        ctx.close()
