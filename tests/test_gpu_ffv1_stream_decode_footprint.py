"""mdvt_decode_video_stream (include/mdvt_ffv1_stream_decode.h) held to its footprint with the arenas of tests/footprint.py, through
the raw C ABI: exactly the first 3 * width bytes of each row of each stored frame, n_packets status words, nothing else; every byte
inside is written; the result does not depend on the bytes behind a packet's end; a refused call leaves everything as it was.  One
far case: packet offsets past 2^32 and a frame_stride past 2^31 (the conventions of tests/test_gpu_far_offsets.py)."""
import ctypes as C

import numpy as np
import pytest

import ffv1_streams as fs
import footprint as fp

pytestmark = pytest.mark.gpu

ENTRY = "mdvt_decode_video_stream"
UNSUPPORTED, INVALID = -3, -1


def _vp(a):
    return C.c_void_p(a.ptr)


@pytest.fixture()
def own_tally():
    try:
        yield
    finally:
        fp.TALLY.pop(ENTRY, None)                      # test_gpu_footprint.py's table lists include/mdvt.h's entry points only


def _stream(rng, k, W, H, N, slices):
    from oracle import ffv1_ref as ref
    frames = fs.stream_content(N, H, W, 100 + k)
    p = ref.Params(coder=k % 2, ec=(k // 2) % 2, intra=0, nh=slices[0], nv=slices[1])
    enc = ref.StreamEncoder(p, W, H, gop=(2, 3, 99)[k % 3])
    return frames, [enc.encode(f) for f in frames], ref.config_record(p)


def test_decode_video_stream_footprint(own_tally):
    import torch
    from metric_depth_video_toolbox_amd import _lib
    from oracle import ffv1_ref as ref
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    try:
        for k, (rng, lays) in enumerate(fp.layout_sweep(8, 570)):
            W = int(rng.choice(fp.WIDTHS[:12]))
            H = int(rng.choice(fp.HEIGHTS[:6]))
            N = 2 + k % 3
            first_out = k % N
            n_out = N - first_out
            order = k % 2
            slices = (min((1, 2, 3, 4)[k % 4], W), min((1, 2, 5)[k % 3], H))
            frames, packets, cfg = _stream(rng, k, W, H, N, slices)
            tail = int(rng.integers(0, 9))             # bytes behind every packet: part of the blob, not of a packet -- they hold poison
            sizes = np.array([len(x) for x in packets], np.uint32)
            offs = np.zeros(N, np.uint64)
            total = 0
            for f in range(N):
                offs[f] = total
                total += len(packets[f]) + tail
            ld, lb, lst = lays.u8(), lays.u8(), fp.Layout(int(rng.choice(fp.BASES4)))
            loff = fp.Layout(int(rng.choice((0, 8))))

            def body(run, bad_cfg=None, short=False, bad_first=None):
                blob = run.out("blob", 1, total, 1, fp.Layout(lb.base, 0, 0))      # poison between the packets ...
                host = blob.read()
                for f in range(N):
                    host[blob.start + int(offs[f]): blob.start + int(offs[f]) + len(packets[f])] = np.frombuffer(packets[f], np.uint8)
                blob.buf.copy_(torch.from_numpy(host))
                blob.input = host[blob.start: blob.start + total].reshape(1, 1, total).copy()      # ... and an input all the same
                o = run.inp("offsets", offs.view(np.uint8).reshape(1, 1, -1), loff)
                s = run.inp("sizes", sizes.view(np.uint8).reshape(1, 1, -1), lst)
                d = run.out("dst", H, 3 * W, n_out, ld)
                st = run.out("status", 1, 4 * N, 1, lst)
                c = bad_cfg if bad_cfg is not None else cfg
                rc = L.mdvt_decode_video_stream(ctx.handle, W, H, c, len(c), _vp(blob), total, _vp(o), _vp(s), N,
                                                first_out if bad_first is None else bad_first, _vp(d),
                                                3 * W - 1 if short else d.pitch, d.stride, order, _vp(st), None)
                if bad_cfg is None and not short and bad_first is None:
                    ctx.check(rc)
                return rc
            tag = f"{W}x{H} x{N} first_out={first_out} slices={slices} order={order} tail={tail} {ld} {lb}"
            out = fp.twice(ENTRY, body, seed=k, what=tag)
            fp.accepted(ENTRY)
            assert not np.ascontiguousarray(out["status"]).view(np.uint32).any(), tag
            want = frames[first_out:, ..., ::-1] if order else frames[first_out:]
            assert np.array_equal(out["dst"].reshape(n_out, H, W, 3), want), tag
            if k % 4 == 0:
                fp.refused(ENTRY, lambda run: body(run, short=True), INVALID, seed=k)
                fp.refused(ENTRY, lambda run: body(run, bad_first=N), INVALID, seed=k)
                fp.refused(ENTRY, lambda run: body(run, bad_first=-1), INVALID, seed=k)
                alpha = ref.config_record(ref.Params(coder=0, intra=0, alpha=1, nh=slices[0], nv=slices[1]))
                fp.refused(ENTRY, lambda run: body(run, bad_cfg=alpha), UNSUPPORTED, seed=k)
        fp.finish_entry(ENTRY)
        t = fp.tally(ENTRY)
        assert t["refused"] >= 8 and t["outside_bytes"] >= 2 * 4096 * t["accepted"]
    finally:
        ctx.close()


def test_decode_video_stream_far(own_tally):
    """Packets 2^31 + delta apart inside d_packets (d_offsets[2] past 2^32) into stored frames 2^31 + delta apart."""
    import torch
    from metric_depth_video_toolbox_amd import _lib
    reason = fp.Slab.skip_reason()
    if reason:
        pytest.skip(reason)
    slab = fp.Slab()
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    try:
        rng = np.random.default_rng(81)
        W, H, N, slices, order, first_out = 33, 9, 4, (2, 2), 1, 1
        frames, packets, cfg = _stream(rng, 0, W, H, N, slices)       # Golomb-Rice, gop 2: keys at 0 and 2
        longest = max(len(p) for p in packets)
        sizes = np.array([len(p) for p in packets], np.uint32)
        ld = fp.Layouts(rng, (1, 3, 1), vec=False).u8()

        def body(run):
            blob = run.out("blob", 1, longest, N, fp.Layout(ld.base, 0, 0))
            host = blob.poison.copy()
            for f in range(N):
                host[blob.pay_index[f, 0, :len(packets[f])]] = np.frombuffer(packets[f], np.uint8)
            slab.put(blob.iv_start, blob.iv_len, host)
            blob.input = host[blob.pay_index].copy()
            offs = np.arange(N, dtype=np.uint64) * np.uint64(blob.stride)
            assert offs[1] > 1 << 31 and offs[2] > 1 << 32
            total = int(offs[-1]) + len(packets[-1])
            o = run.inp("offsets", offs.view(np.uint8).reshape(1, 1, -1), fp.Layout(8))
            s = run.inp("sizes", sizes.view(np.uint8).reshape(1, 1, -1))
            d, st = run.out("dst", H, 3 * W, N - first_out, ld), run.out("status", 1, 4 * N)
            assert d.stride > 1 << 31
            ctx.check(L.mdvt_decode_video_stream(ctx.handle, W, H, cfg, len(cfg), _vp(blob), total, _vp(o), _vp(s), N, first_out, _vp(d),
                                                 d.pitch, d.stride, order, _vp(st), None))
        with fp.far(fp.Far(slab, "stride")):
            out = fp.twice(ENTRY, body, seed=3, what=f"{W}x{H} x{N}")
        assert not np.ascontiguousarray(out["status"]).view(np.uint32).any()
        assert np.array_equal(out["dst"].reshape(N - first_out, H, W, 3), frames[first_out:, ..., ::-1])
    finally:
        ctx.close()
        del slab.buf
        torch.cuda.empty_cache()
