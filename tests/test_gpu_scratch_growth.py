"""Every scratch block of a context walked through growth, and all of them handed back by mdvt_destroy.

A context keeps one block of device memory per kind of call that needs scratch (the hole-count buffers, the multisample and
near-clip key planes, the workspaces of the normal infill, of both infill-mask completions, of the FFV1 encoder and decoder and of
the convergence depths).  A block is sized by the largest call so far: it grows when a larger call comes and never shrinks.  One
context lives through all of them here.  Per scratch user three calls: a small one on stream A, a larger one on stream B with no
host synchronisation in between (growing has to wait for the small call itself: its block goes back to the pool), the small one
again on A (ordered behind B on the device: a context's scratch serves one stream at a time, mdvt.h).

Asserted: every output of every call equals, byte for byte, the same call on a fresh context; mdvt_workspace_bytes never falls
and is after the third call what it was after the second; and closing the context raises the pool's idle bytes by exactly the
context's mdvt_workspace_bytes -- a block mdvt_destroy forgot would be missing from the rise.  Public API only.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_context_reuse import GREEN, apply_cfg, base_cfg, frame_pool, ni_inputs, synthetic_seed

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

W, H = 64, 48          # growth does not depend on the frame's shape; W % 4 == 0 keeps the vector paths in play


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from metric_depth_video_toolbox_amd import _lib, ffv1_device, stereo_rerender, synthetic, video_io
    return _lib, stereo_rerender, synthetic, ffv1_device, video_io


class Inputs:
    """Device inputs of every call, made once, before anything is launched."""

    def __init__(self, mods):
        _lib, sr, synthetic, fd, video_io = mods
        rng = np.random.default_rng(11)
        depth, color = frame_pool(synthetic, W, H, rng, n=6)
        self.depth, self.color = torch.from_numpy(depth).cuda(), torch.from_numpy(color).cuda()
        pairs = [ni_inputs(rng, color[k]) for k in range(6)]
        self.ni_img = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
        self.ni_mask = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
        self.ni_hole = torch.from_numpy(np.stack([np.any(p[1] != 0, -1).astype(np.uint8) * 255 for p in pairs])).cuda()
        seeds = np.stack([synthetic_seed(rng, W, H, GREEN) for _ in range(6)])
        self.seed = torch.from_numpy(seeds).cuda()
        self.seed_sbs = torch.from_numpy(np.concatenate([seeds[:3], seeds[3:]], axis=2)).cuda()       # [3, H, 2W, 3]
        # FFV1: the frames, and their packets from the host encoder in both slice layouts
        self.packets = {sl: [video_io.encode_frame(color[k], slices=sl)[0] for k in range(4)] for sl in ((1, 1), (4, 4))}
        self.ffv1_cfg = {sl: video_io.encode_frame(color[0], slices=sl)[1] for sl in ((1, 1), (4, 4))}
        torch.cuda.synchronize()


def _render(r, inp, n, **want):
    """A batch of n pure-shift frames; the outputs in a fixed order."""
    res = r.prepare(inp.depth[:n].contiguous(), inp.color[:n].contiguous(), [r.frame_params(xfov=45.0)] * n, **want)
    res.launch(torch.cuda.current_stream())
    return [res.results[k] for k in sorted(res.results)]


def _normal_infill(r, inp, n):
    out = torch.empty_like(inp.ni_img[:n])
    r.ctx.check(r._L.mdvt_normal_infill(r.ctx.handle, inp.ni_img.data_ptr(), 3 * W, 3 * W * H, inp.ni_mask.data_ptr(), 3 * W, 3 * W * H,
                                        out.data_ptr(), 3 * W, 3 * W * H, n, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return [out]


def _mask_normals(r, inp, n):
    img = inp.ni_img[:n].clone()                       # (filled in place)
    r.ctx.check(r._L.mdvt_infill_using_mask_normals(r.ctx.handle, img.data_ptr(), 3 * W, 3 * W * H, inp.ni_hole.data_ptr(), W, W * H,
                                                    inp.ni_mask.data_ptr(), 3 * W, 3 * W * H, n, 400,
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return [img]


def _convergence(r, inp, masked):
    n = 4 if masked else 2
    means = torch.empty(n, dtype=torch.float32, device="cuda")
    counts = torch.empty(n, dtype=torch.int32, device="cuda")
    d, m = inp.depth[:n].contiguous(), inp.color[:n].contiguous()       # (any image serves as a mask: its nonzero pixels select)
    r.ctx.check(r._L.mdvt_convergence_depths(r.ctx.handle, W, H, d.data_ptr(), 3 * W, 3 * W * H, 0, m.data_ptr() if masked else None,
                                             3 * W if masked else 0, 3 * W * H if masked else 0, 0, n, n if masked else 0, 100.0,
                                             means.data_ptr(), counts.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return [means.view(torch.int32), counts]


def _encode(mods, r, inp, n, slices):
    p = mods[3].enqueue(r.ctx, inp.color[:n].contiguous(), slices=slices)
    return [p.packets, p.offsets, p.sizes], p


def _decode(mods, r, inp, n, slices):
    p = mods[3].enqueue_decode(r.ctx, inp.packets[slices][:n], inp.ffv1_cfg[slices], W, H)
    return [p.out, p.status], p


def users(mods):
    """(name, configuration of the context, the call) per scratch user; call(r, inp, large) -> output tensors (the call is only
    enqueued, on the current stream) or (tensors, what finishes them)."""
    return [
        ("normal_infill", {}, lambda r, inp, large: _normal_infill(r, inp, 5 if large else 1)),
        # (the same block as normal_infill's: six images, so that this one grows it too -- a large call that found the block large
        #  enough would run beside the small one on the other stream, in the same scratch)
        ("infill_using_mask_normals", {}, lambda r, inp, large: _mask_normals(r, inp, 6 if large else 1)),
        ("finish_infill_mask", dict(key=GREEN),
         lambda r, inp, large: list(r.finish_infill_mask_sbs(inp.seed_sbs, max_rounds=300, want_remaining=True)) if large
         else list(r.finish_infill_mask(inp.seed[:1], max_rounds=8, want_remaining=True))),
        ("finish_infill_mask_heap", dict(key=GREEN),
         lambda r, inp, large: list(r.finish_infill_mask_sbs(inp.seed_sbs[:2], want_remaining=True, order="heap")) if large
         else list(r.finish_infill_mask(inp.seed[:1], want_remaining=True, order="heap"))),
        ("encode_video_frames", {}, lambda r, inp, large: _encode(mods, r, inp, 4 if large else 1, (4, 4) if large else (1, 1))),
        ("decode_video_frames", {}, lambda r, inp, large: _decode(mods, r, inp, 4 if large else 1, (4, 4) if large else (1, 1))),
        ("convergence_depths", {}, lambda r, inp, large: _convergence(r, inp, large)),
        ("render with hole counts", dict(mesh=False), lambda r, inp, large: _render(r, inp, 6 if large else 1, want_hole_counts=True)),
        ("render with samples = 4", dict(samples=4), lambda r, inp, large: _render(r, inp, 3 if large else 1)),
        ("mesh render with near-plane clipping", dict(near_clip=1), lambda r, inp, large: _render(r, inp, 3 if large else 1)),
    ]


def _finish(res):
    """Output tensors of a call -> their bytes on the host (after the caller has synchronised)."""
    tensors, pending = res if isinstance(res, tuple) else (res, None)
    if pending is not None and hasattr(pending, "collect"):
        got = pending.collect()
        if isinstance(got, list):                      # the encoder's packets: what was written of the packet buffer
            assert pending.host_frames == 0
            return [np.frombuffer(b"".join(got), np.uint8), tensors[2].cpu().numpy()]
        assert not pending.flags.any() and pending.host_frames == 0
    return [t.cpu().numpy() for t in tensors]


def test_every_scratch_block_grows_and_is_returned(mods):
    _lib, sr = mods[0], mods[1]
    inp = Inputs(mods)

    def fresh(cfg, call, large):
        r = sr.StereoRerenderer(W, H, pupillary_distance=65)
        try:
            apply_cfg(_lib, r, cfg)
            res = call(r, inp, large)
            torch.cuda.synchronize()
            return _finish(res)
        finally:
            r.close()

    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    live = sr.StereoRerenderer(W, H, pupillary_distance=65)
    try:
        seen = [live.ctx.workspace_bytes()]
        for name, over, call in users(mods):
            cfg = base_cfg(**over)
            want = {large: fresh(cfg, call, large) for large in (False, True)}
            apply_cfg(_lib, live, cfg)
            steps = []
            for k, (stream, large) in enumerate(((a, False), (b, True), (a, False))):
                if k == 2:
                    a.wait_stream(b)
                with torch.cuda.stream(stream):
                    steps.append((large, call(live, inp, large)))
                seen.append(live.ctx.workspace_bytes())
                assert seen[-1] >= seen[-2], f"{name}, call {k}: mdvt_workspace_bytes fell from {seen[-2]} to {seen[-1]}"
            assert seen[-1] == seen[-2], f"{name}: the small call after the large one changed mdvt_workspace_bytes {seen[-2]} -> {seen[-1]}"
            torch.cuda.synchronize()
            for k, (large, res) in enumerate(steps):
                got = _finish(res)
                assert len(got) == len(want[large])
                for j, (g, w) in enumerate(zip(got, want[large])):
                    assert g.shape == w.shape and np.array_equal(g, w), f"{name}, call {k}: output {j} differs from a fresh context's"
        print("mdvt_workspace_bytes after each call:", seen)
        _lib.release_cached_memory()
        idle0 = _lib.cached_memory()[0]
        held = live.ctx.workspace_bytes()
        assert held > 0
        live.close()
        assert _lib.cached_memory()[0] - idle0 == held, "mdvt_destroy did not hand every block of the context back to the pool"
    finally:
        torch.cuda.synchronize()
        live.close()
