"""mdvt_convergence_depths (include/mdvt_convergence.h) held to its footprint with the arenas of tests/footprint.py, through the raw
C ABI: exactly n_frames floats and, where given, n_frames words, nothing else; every one of them is written; the result does not
depend on the bytes behind the first 3 * width of a row; a refused call leaves everything as it was.  (The entry point is declared
outside include/mdvt.h, so its case family lives here and not in test_gpu_footprint.py; its tally row is printed here and taken out
of the shared table again.)"""
import ctypes as C

import numpy as np
import pytest

import convergence_ref as cr
import footprint as fp

pytestmark = pytest.mark.gpu

ENTRY = "mdvt_convergence_depths"
UNSUPPORTED, INVALID = -3, -1


def _vp(a):
    return C.c_void_p(a.ptr)


@pytest.fixture()
def own_tally():
    try:
        yield
    finally:
        fp.TALLY.pop(ENTRY, None)                      # test_gpu_footprint.py's table lists include/mdvt.h's entry points only


def test_convergence_depths_footprint(own_tally):
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    try:
        vector = 0
        for k, (rng, lays) in enumerate(fp.layout_sweep(10, 920)):
            W = int(rng.choice(fp.WIDTHS))
            H = int(rng.choice(fp.HEIGHTS + (40, 67)))     # (257 x 40, 250 x 67: more than one chunk of 8192)
            if lays.vec:
                W = max(8, W & ~3)
            N = 1 + k % 3
            M = (k // 2) % (N + 1)                         # mask frames: none, some, all
            order = k % 2
            with_counts = k % 3 != 1
            depth = cr.random_depth(rng, N, H, W)
            mask = np.repeat(rng.choice(np.array([0, 240, 241, 255], np.uint8), (max(M, 1), H, W, 1)), 3, axis=3)
            if M and k % 5 == 0:
                mask[0] = 3                                # an empty selection: its NaN is written too
            want, n = cr.clip_means(depth, mask[:M] if M else None)
            ld, lm, lo, lc = lays.u8(), lays.u8(), lays.w32(), lays.w32()

            def body(run, short=False, bad_mask=False):
                d = run.inp("depth", (depth[..., ::-1] if order else depth).reshape(N, H, 3 * W), ld)
                m = run.inp("mask", (mask[..., ::-1] if order else mask).reshape(len(mask), H, 3 * W), lm)
                o = run.out("means", 1, 4 * N, 1, fp.Layout(lo.base))
                c = run.out("counts", 1, 4 * N, 1, fp.Layout(lc.base))
                rc = L.mdvt_convergence_depths(ctx.handle, W, H, _vp(d), 3 * W - 1 if short else d.pitch, d.stride, order,
                                               _vp(m) if M else None, m.pitch, m.stride, order, N, N + 1 if bad_mask else M, 100.0,
                                               _vp(o), _vp(c) if with_counts else None, None)
                if not short and not bad_mask:
                    ctx.check(rc)
                # the 12-byte loads of four pixels: row length (all W * H pixels where the rows have no padding), base, pitch and stride of
                # a video all multiples of 4
                run.vector = all((W * H if a.pitch == 3 * W else W) % 4 == 0 and a.ptr % 4 == 0 and a.pitch % 4 == 0 and a.stride % 4 == 0
                                 for a in [d] + ([m] if M else []))
                return rc
            tag = f"{W}x{H} x{N} mask frames {M} order={order} counts={with_counts} {ld} {lm}"

            def body_accepted(run):
                body(run)
                if not with_counts:                        # d_counts NULL: the arena stays poison, as an input would
                    run.arenas["counts"].input = run.arenas["counts"].payload(run.arenas["counts"].poison)
                body_accepted.vector = run.vector
            out = fp.twice(ENTRY, body_accepted, seed=k, what=tag)
            _, _, v = fp.accepted(ENTRY, vector=body_accepted.vector)
            vector += int(body_accepted.vector)
            got = np.ascontiguousarray(out["means"]).view(np.float32).reshape(N)
            assert cr.same_bits(got, want).size == 0, f"{tag}: {got} vs {want}"
            if with_counts:
                assert np.ascontiguousarray(out["counts"]).view(np.uint32).reshape(N).tolist() == n.tolist(), tag
            if k % 4 == 0:
                fp.refused(ENTRY, lambda run: body(run, short=True), INVALID, seed=k)
                fp.refused(ENTRY, lambda run: body(run, bad_mask=True), INVALID, seed=k)
        fp.finish_entry(ENTRY)
        t = fp.tally(ENTRY)
        assert vector >= 2, "no layout reached the 12-byte loads"
        assert t["refused"] >= 4 and t["outside_bytes"] >= 2 * 4096 * t["accepted"]
    finally:
        ctx.close()
