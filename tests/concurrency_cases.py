"""Case material of tests/test_gpu_concurrency.py: nine families of small calls, each built from material the suite already owns
(the scenes, seeds, streams and inputs of the single-threaded tests of that family), each with expected values that are an
oracle's or a reference's, computed once on the main thread (build) before any worker thread exists.  A Worker runs a seeded
schedule of such calls on a stream, contexts and renderers of its own and compares every output byte for byte; the same code runs
the schedules one after the other (the control) and in four threads at once.  Plain module: no fixture, no pytest setting."""
import ctypes as C
import threading
import time

import numpy as np
import torch

import convergence_ref as cr
import ffv1_streams as fs
import ffv1_ycbcr_ref as yr
import metric_align_ref as mr
from test_gpu_context_reuse import GREEN, _default_bits, apply_cfg, base_cfg, check_frame, fmm_finish, frame_pool, oracle_frame
from test_gpu_convergence import _batch as convergence_batch, _raw as raw_convergence
from test_gpu_ffv1_encode import _content as encode_content
from test_gpu_metric_align import _raw_fit as raw_fit

FAMILIES = ("points", "mesh_banks", "completion", "normal_infill", "ffv1_encode", "ffv1_stream", "ffv1_ycbcr", "fit_codes", "convergence")
# (variants of a family, smaller first -- a worker's "grow" step runs smaller, larger, smaller on fresh contexts)
VARIANTS = {"points": ("64x32", "61x33"), "mesh_banks": ("250x61x9",), "completion": ("waiting", "no_host_wait", "heap"),
            "normal_infill": ("noise", "blobs"), "ffv1_encode": ("33x17",), "ffv1_stream": ("rgb_golomb",), "ffv1_ycbcr": ("yuv420p",),
            "fit_codes": ((1, 3, 43), (5, 41, 83)), "convergence": ("1x205x83", "5x205x83")}
GROWS = ("fit_codes", "convergence")                          # the families whose calls come in two sizes: their scratch block grows
YCBCR_CASE = (64, 48, 7, "yuv420p", 0, 1, 3, 0, (2, 2), 3)
DEFAULT_LIMIT = 4 << 30                                       # mdvt_set_cached_memory_limit's default (include/mdvt.h)
POISON = 0xA5


def poisoned(shape, dtype=torch.uint8):
    """An output buffer as every call here gets it: 0xA5 bytes, -7.0 for floats."""
    return torch.full(tuple(shape), -7.0 if dtype == torch.float32 else (POISON if dtype == torch.uint8 else -7), dtype=dtype, device="cuda")


def _aux_masks(rng, W, H):
    """The two normal-mask kinds of test_gpu_render.py::test_randomised_aux_sweep: noise (every pixel its own direction, zero
    channels at random) and a few blobs of coherent directions."""
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    noise[rng.uniform(size=(H, W)) < rng.uniform(0.2, 0.95)] = 0
    noise[rng.uniform(size=(H, W)) < 0.05, int(rng.integers(3))] = 0
    yy, xx = np.mgrid[0:H, 0:W]
    keep = np.zeros((H, W), bool)
    for _ in range(3):
        keep |= (xx - rng.uniform(0, W)) ** 2 + (yy - rng.uniform(0, H)) ** 2 < rng.uniform(1, max(2.0, max(W, H) / 3)) ** 2
    base = rng.integers(1, 256, 3)
    blobs = np.clip(base[None, None, :] + rng.integers(-6, 7, (H, W, 3)), 1, 255).astype(np.uint8)
    blobs[~keep] = 0
    return {"noise": noise, "blobs": blobs}


class Material:
    """Inputs on the device and expected values on the host, per family and variant.  Read-only once built."""

    def __init__(self, orc):
        from metric_depth_video_toolbox_amd import stereo_rerender as sr, synthetic, video_io
        self.orc = orc
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        # ---- points, pure shift: the frame pool of the context walks, both grids
        self.points = {}
        for name, (W, H) in zip(VARIANTS["points"], ((64, 32), (61, 33))):
            d, c = frame_pool(synthetic, W, H, np.random.default_rng(W * 100 + H), n=3)
            p = sr.make_frame_params(W, H, xfov=45.0, pupillary_distance=65)
            want = {bits: [oracle_frame(orc, W, H, base_cfg(mesh=False, bits=bits), p, None, d[k], c[k]) for k in range(len(d))]
                    for bits in (0, 4)}
            self.points[name] = dict(W=W, H=H, d=up(d), c=up(c), p=p, want=want)
        # ---- mesh, posed / converged, launch sets on two banks: test_gpu_render.py::test_two_banks_on_other_shapes' first case
        W, H, N = 250, 61, 9
        d, c = synthetic.SyntheticScene(W, H, seed=W + N, n_fg=5).clip(N)
        T = synthetic.synthetic_pose_track(N + 8)
        Ts = [T[k + 2] if k % 2 else None for k in range(N)]
        ps = [sr.make_frame_params(W, H, xfov=50.0, pupillary_distance=65, convergence_distance=None if k % 2 else 2.2, transformation=Ts[k])
              for k in range(N)]
        want = {bits: [oracle_frame(orc, W, H, base_cfg(mesh=True, bits=bits), ps[k], Ts[k], d[k], c[k], want_depth=True) for k in range(N)]
                for bits in (0, 4)}
        self.mesh = dict(W=W, H=H, N=N, d=up(d), c=up(c), ps=ps, want=want)
        # ---- points with edge removal -> seed -> completion (test_gpu_inpaint_heap.py's composition for the heap order)
        W, H = 96, 64
        d, c = frame_pool(synthetic, W, H, np.random.default_rng(9664), n=2)
        p = sr.make_frame_params(W, H, xfov=45.0, pupillary_distance=65)
        cfg = base_cfg(mesh=False, rm=True, ep=1, key=GREEN, bits=_default_bits())
        frames = [oracle_frame(orc, W, H, cfg, p, None, d[k], c[k], want_seed=True) for k in range(len(d))]
        levels = [[orc.finish_infill_mask(f[eye + "_seed"], key_rgb=GREEN, max_rounds=W + H) for eye in ("left", "right")] for f in frames]
        heap = [[fmm_finish(orc, f[eye + "_seed"], GREEN) for eye in ("left", "right")] for f in frames]
        self.completion = dict(W=W, H=H, d=up(d), c=up(c), p=p, cfg=cfg, frames=frames, levels=levels, heap=heap)
        # ---- normal_infill and infill_using_mask_normals: 100 x 31, both mask kinds of the aux sweep
        W, H = 100, 31
        rng = np.random.default_rng(10031)
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        self.normal = {}
        for kind, mask in _aux_masks(rng, W, H).items():
            nimg = img.copy()
            nimg[rng.uniform(size=(H, W)) < 0.1] = 0
            hole = np.any(mask != 0, -1)
            himg = img.copy()
            himg[hole] = 0
            wn = ((mask.astype(np.float32) / np.float32(255.0)) * 2 - 1).astype(np.float32)
            self.normal[kind] = dict(W=W, H=H, img=up(nimg), mask=up(mask), himg=up(himg), hole=up(hole.astype(np.uint8) * 255),
                                     want_ni=orc.normal_infill(nimg, mask), want_mn=orc.infill_using_normals(himg, hole, wn))
        # ---- FFV1 encode: 33 x 17, slices (4, 4), three content kinds
        W, H = 33, 17
        rng = np.random.default_rng(W * 1000 + H)
        frames = np.stack([encode_content(kind, W, H, rng, t) for t, kind in enumerate(("gradient", "synthetic", "noise"))])
        self.encode = dict(frames=up(frames), want=[video_io.encode_frame(np.ascontiguousarray(f), slices=(4, 4))[0] for f in frames])
        # ---- FFV1 stream decode: RGB Golomb-Rice with inter frames, and yuv420p
        W, H, N = fs.COUNTERS_CASE[:3]
        frames, packets, cfg = fs.make_stream(fs.COUNTERS_CASE)
        self.stream = dict(W=W, H=H, N=N, packets=list(packets), cfg=cfg, want=frames)
        assert YCBCR_CASE in yr.MATRIX
        W, H, N = YCBCR_CASE[:3]
        _planes, rgb, packets, cfg = yr.make_stream(YCBCR_CASE)
        self.ycbcr = dict(W=W, H=H, N=N, packets=list(packets), cfg=cfg, want=rgb)
        # ---- fit, then the codes behind it on the same stream
        self.fit = {}
        cases = {(5, 41, 83): [c for c in mr.FIT_INPUTS["every_size"] if c[1] == (5, 41, 83)][0],
                 (1, 3, 43): [c for c in mr.FIT_INPUTS["growth"] if c[1] == (1, 3, 43)][0]}
        for shape in VARIANTS["fit_codes"]:
            p, d, _ = mr.fit_input(*cases[shape])
            want = mr.fit(mr.concat(p), mr.concat(mr.inverse(d)))
            codes, _depth = mr.metric_codes(p, want[5], want[6], 100, 0)
            self.fit[shape] = dict(p=up(p), d=up(d), want=want, codes=codes)
        # ---- convergence depths: test_gpu_convergence.py's batch of 5 with 3 mask frames, one of them selecting nothing; and one
        # unmasked frame (the smaller call of the family)
        W, H = 205, 83
        self.convergence = {}
        for name, (n, n_mask, empty, seed) in zip(VARIANTS["convergence"], ((1, 0, None, 1), (5, 3, 1, 5))):
            depth, mask = convergence_batch(np.random.default_rng(seed), n, n_mask, H, W, empty=empty)
            means, counts = cr.clip_means(depth, mask if n_mask else None)
            self.convergence[name] = dict(d=up(depth), m=up(mask) if n_mask else None, n_mask=n_mask, want=means, counts=counts)
        torch.cuda.synchronize()


def schedule(index, steps, seed0=20261019):
    """Worker `index`'s steps, drawn from its seed alone: (family, variant index, action, through).  action: None, "recreate" (close a
    renderer or the context first), "grow" (fresh contexts; the family's smaller call, the larger, the smaller) or "switch" (the
    renderer's sub-pixel grid 0 <-> 4, or its workspace budget).  through: "own" (the worker's own Context through a face that
    takes one) or "face" (a Python face, which reaches the thread's shared context)."""
    rng = np.random.default_rng(seed0 + index)
    out = []
    order = list(rng.permutation(len(FAMILIES)))             # every family at least once (from 9 steps on), then at random
    for k in range(steps):
        fam = FAMILIES[order[k] if k < len(order) else int(rng.integers(len(FAMILIES)))]
        action = None
        roll = int(rng.integers(8))
        if roll == 0:
            action = "recreate"
        elif roll == 1 and fam in GROWS:
            action = "grow"
        elif roll in (2, 3) and fam in ("points", "mesh_banks"):
            action = "switch"
        out.append((fam, int(rng.integers(len(VARIANTS[fam]))), action, "own" if rng.integers(2) else "face"))
    return out


class Worker:
    """One schedule on a stream, contexts and renderers of its own.  run() is the thread's body (and the control's): it never raises;
    the first failure is kept in .error with its tag, the steps' host intervals in .log."""

    def __init__(self, mat, index, steps, barrier=None, gate=None):
        """gate(step), if given, is called in front of every step, outside the step's interval (the pool test's rendezvous)."""
        self.mat, self.index, self.steps, self.barrier, self.gate = mat, index, schedule(index, steps), barrier, gate
        self.log, self.error, self.done = [], None, False
        self.renderers, self.cfgs, self.ctxs, self.stream = {}, {}, {}, None
        self.statuses = []
        self.growth = []                      # per "grow" step: (family, workspace bytes of the own context after each of its calls)

    # -- contexts ---------------------------------------------------------------------------------
    def renderer(self, key, W, H, cfg, **kw):
        from metric_depth_video_toolbox_amd import stereo_rerender as sr
        if key not in self.renderers:
            self.renderers[key] = sr.StereoRerenderer(W, H, pupillary_distance=65, subpixel_bits=cfg["bits"], **kw)
            self.cfgs[key] = dict(cfg)
        return self.renderers[key], self.cfgs[key]

    def own_ctx(self, W=16, H=16):
        """The worker's own plain Context: 16 x 16 for the codec, fit and convergence calls, the image's size for the normal infill
        (whose entry points take the image size from the context)."""
        from metric_depth_video_toolbox_amd import _lib
        if (W, H) not in self.ctxs:
            self.ctxs[W, H] = _lib.Context(0, W, H)
        return self.ctxs[W, H]

    def close_ctxs(self):
        for ctx in self.ctxs.values():
            ctx.close()
        self.ctxs.clear()

    def recreate(self, rng_pick):
        """Closes the contexts or one renderer (the stream is idle: every step ends synchronised); the next use makes a new one."""
        keys = sorted(self.renderers)
        if keys and rng_pick % (len(keys) + 1):
            key = keys[rng_pick % len(keys)]
            self.renderers.pop(key).close()
            self.cfgs.pop(key)
        else:
            self.close_ctxs()

    def close(self):
        for r in self.renderers.values():
            r.close()
        self.renderers.clear()
        self.close_ctxs()

    # -- the thread -------------------------------------------------------------------------------
    def run(self):
        try:
            self.stream = torch.cuda.Stream()
            with torch.cuda.stream(self.stream):
                if self.barrier is not None:
                    self.barrier.wait(timeout=60)
                for step, (fam, variant, action, through) in enumerate(self.steps):
                    tag = f"thread {self.index} step {step} {fam}/{VARIANTS[fam][variant]} action={action} through={through}"
                    try:
                        if self.gate is not None:
                            self.gate(step)
                        if action == "recreate":
                            self.recreate(step)
                        if action == "grow":
                            # fresh contexts: the smaller call sizes the scratch block, the larger one grows it -- behind a device
                            # synchronisation, while the other threads enqueue -- and the smaller one follows the larger
                            self.close()
                            todo = [(0, "own"), (1, "own"), (0, "own")]
                        else:
                            todo = [(variant, through)]
                        sizes = []
                        for v, thr in todo:
                            t_enter = time.perf_counter()
                            check = getattr(self, "step_" + fam)(v, thr, action)
                            self.stream.synchronize()
                            t_exit = time.perf_counter()
                            check()
                            self.log.append((self.index, step, fam, t_enter, t_exit))
                            if action == "grow":
                                sizes.append(self.own_ctx().workspace_bytes())
                        if action == "grow":
                            self.growth.append((fam, tuple(sizes)))
                    except BaseException as e:                      # noqa: BLE001
                        self.error = (tag, e)
                        return
                self.stream.synchronize()
        except BaseException as e:                                  # noqa: BLE001
            self.error = (f"thread {self.index} outside its steps", e)
        finally:
            try:
                self.close()
            except BaseException as e:                              # noqa: BLE001
                self.error = self.error or (f"thread {self.index} closing its contexts", e)
            self.done = True

    # -- the families: each enqueues on the current stream and returns the comparison to run once the stream is idle ---------------
    def step_points(self, v, through, action):
        from metric_depth_video_toolbox_amd import _lib
        name = VARIANTS["points"][v]
        m = self.mat.points[name]
        W, H = m["W"], m["H"]
        r, cfg = self.renderer(("points", name), W, H, base_cfg(mesh=False, bits=_default_bits() if _default_bits() in (0, 4) else 0),
                               render_as_pointcloud=True)
        if action == "switch":
            cfg["bits"] = 4 - cfg["bits"]
            apply_cfg(_lib, r, cfg)
        N = int(m["d"].shape[0])
        # a width that is a multiple of 4 takes the fused path (16-byte loads; the packed mask is the only mask), any other the byte path
        fused = W % 4 == 0
        got = r.render(m["d"], m["c"], [m["p"]] * N, out_sbs=poisoned((N, H, 2 * W, 3)), out_mask=None if fused else poisoned((N, H, 2 * W)),
                       want_maskbits=True, want_hole_counts=True, want_mask=not fused)
        want, tag = m["want"][cfg["bits"]], f"points {name} bits={cfg['bits']}"

        def check():
            for f in range(N):
                check_frame(got, f, want[f], W, f"{tag} frame {f}")
        return check

    def step_mesh_banks(self, v, through, action):
        from metric_depth_video_toolbox_amd import _lib
        m = self.mat.mesh
        W, H, N = m["W"], m["H"], m["N"]
        r, cfg = self.renderer(("mesh",), W, H, base_cfg(mesh=True, bits=_default_bits() if _default_bits() in (0, 4) else 0, ws_mib=8),
                               workspace_mib=8)
        if action == "switch":
            if self.index % 2:
                cfg["bits"] = 4 - cfg["bits"]
            else:
                cfg["ws_mib"] = 13 - cfg["ws_mib"]              # 8 <-> 5 MiB: launch sets of another length, the same frames
            apply_cfg(_lib, r, cfg)
        got = r.render(m["d"], m["c"], m["ps"], out_sbs=poisoned((N, H, 2 * W, 3)), out_mask=poisoned((N, H, 2 * W)), want_depth=True,
                       out_depth=poisoned((N, H, 2 * W), torch.float32))
        want, tag = m["want"][cfg["bits"]], f"mesh on two banks bits={cfg['bits']} ws_mib={cfg['ws_mib']}"

        def check():
            for f in range(N):
                check_frame(got, f, want[f], W, f"{tag} frame {f}")
        return check

    def step_completion(self, v, through, action):
        form = VARIANTS["completion"][v]
        m = self.mat.completion
        W, H = m["W"], m["H"]
        r, _cfg = self.renderer(("completion",), W, H, m["cfg"], render_as_pointcloud=True, infill_mask=True)
        N = int(m["d"].shape[0])
        got = r.render(m["d"], m["c"], [m["p"]] * N, out_sbs=poisoned((N, H, 2 * W, 3)), out_mask=poisoned((N, H, 2 * W)), want_seed=True)
        out = poisoned((N, H, 2 * W, 3))
        if form == "heap":
            r.finish_infill_mask_sbs(got["seed"], out=out, order="heap")
            rem = None
        else:
            _, rem = r.finish_infill_mask_sbs(got["seed"], out=out, max_rounds=W + H, want_remaining=True, no_host_wait=form == "no_host_wait")

        def check():
            img = out.cpu().numpy()
            for f in range(N):
                check_frame(got, f, m["frames"][f], W, f"completion ({form}): the render in front of it, frame {f}")
                for e in range(2):
                    if form == "heap":
                        assert np.array_equal(img[f, :, e * W:(e + 1) * W], m["heap"][f][e]), f"completion (heap) frame {f} eye {e} differs"
                    else:
                        wimg, wrem = m["levels"][f][e]
                        assert np.array_equal(img[f, :, e * W:(e + 1) * W], wimg), f"completion ({form}) frame {f} eye {e} differs"
                        assert int(rem[e, f]) == wrem, f"completion ({form}) frame {f} eye {e}: remaining {int(rem[e, f])} != {wrem}"
        return check

    def step_normal_infill(self, v, through, action):
        from metric_depth_video_toolbox_amd import basic_nomal_infill, stereo_rerender as sr
        kind = VARIANTS["normal_infill"][v]
        m = self.mat.normal[kind]
        H, W = m["H"], m["W"]
        out_ni, out_mn = poisoned((H, W, 3)), poisoned((H, W, 3))
        if through == "own":          # the C entry points on the worker's own context, as the context walks call them
            ctx, s = self.own_ctx(W, H), C.c_void_p(torch.cuda.current_stream().cuda_stream)
            ctx.call("mdvt_normal_infill", m["img"].data_ptr(), 3 * W, 0, m["mask"].data_ptr(), 3 * W, 0, out_ni.data_ptr(), 3 * W, 0, 1, s)
            out_mn.copy_(m["himg"])
            ctx.call("mdvt_infill_using_mask_normals", out_mn.data_ptr(), 3 * W, 0, m["hole"].data_ptr(), W, 0, m["mask"].data_ptr(), 3 * W, 0,
                     1, 400, s)
        else:
            basic_nomal_infill.normal_infill(m["img"], m["mask"], out=out_ni)
            sr.infill_using_mask_normals(m["himg"], m["hole"], m["mask"], out=out_mn)

        def check():
            assert np.array_equal(out_ni.cpu().numpy(), m["want_ni"]), f"normal_infill ({kind}, {through}) differs"
            assert np.array_equal(out_mn.cpu().numpy(), m["want_mn"]), f"infill_using_mask_normals ({kind}, {through}) differs"
        return check

    def step_ffv1_encode(self, v, through, action):
        from metric_depth_video_toolbox_amd import ffv1_device as fd
        m = self.mat.encode
        p = fd.enqueue(self.own_ctx() if through == "own" else fd._context(0), m["frames"], slices=(4, 4))

        def check():
            got = p.collect()
            assert p.host_frames == 0, "a frame was coded on the host"
            assert got == m["want"], f"FFV1 packets ({through}) differ in frames {[k for k, (a, b) in enumerate(zip(got, m['want'])) if a != b]}"
        return check

    def _decode(self, m, through, what):
        from metric_depth_video_toolbox_amd import ffv1_device as fd
        n = m["N"]
        out = poisoned((n, m["H"], m["W"], 3))
        p = fd.enqueue_decode_stream(self.own_ctx() if through == "own" else fd._context(0), m["packets"], m["cfg"], m["W"], m["H"], out=out)

        def check():
            frames = p.collect().cpu().numpy()
            assert p.host_frames == 0 and not p.flags.any(), f"{what} ({through}): status {p.flags.tolist()}, {p.host_frames} frames on the host"
            assert np.array_equal(frames, m["want"]), f"{what} ({through}): frames differ"
        return check

    def step_ffv1_stream(self, v, through, action):
        return self._decode(self.mat.stream, through, "RGB Golomb-Rice stream")

    def step_ffv1_ycbcr(self, v, through, action):
        return self._decode(self.mat.ycbcr, through, "yuv420p stream")

    def step_fit_codes(self, v, through, action):
        from metric_depth_video_toolbox_amd import _lib, video_metric_convert as vmc
        shape = VARIANTS["fit_codes"][v]
        m = self.mat.fit[shape]
        N, H, W = shape
        if through == "own":
            ctx = self.own_ctx()
            values = poisoned((8,), torch.float32)
            rc = raw_fit(_lib, ctx, m["p"], m["d"], None, values, tid=1, stream=torch.cuda.current_stream())
            self.statuses.append(rc)
            ctx.check(rc)
        else:
            values = vmc.compute_scale_and_shift_full(m["p"], m["d"], target_is_depth=True).values
        codes = vmc.metric_depth_codes(m["p"], values, 100, out=poisoned((N, H, W, 3)))      # behind the fit, on the same stream

        def check():
            got = values.cpu().numpy()
            bad = mr.same_bits(got, m["want"])
            assert bad.size == 0, f"fit {shape} ({through}): floats {bad.tolist()} differ: got {got.tolist()} want {m['want'].tolist()}"
            assert np.array_equal(codes.cpu().numpy(), m["codes"]), f"codes behind the fit {shape} ({through}) differ"
        return check

    def step_convergence(self, v, through, action):
        from metric_depth_video_toolbox_amd import _lib, find_convergence_depth as fcd
        m = self.mat.convergence[VARIANTS["convergence"][v]]
        N = int(m["d"].shape[0])
        if through == "own":
            ctx = self.own_ctx()
            means, counts = poisoned((N,), torch.float32), poisoned((N,), torch.int32)
            rc = raw_convergence(_lib, ctx, m["d"], m["m"], m["n_mask"], means, counts, stream=torch.cuda.current_stream())
            self.statuses.append(rc)
            ctx.check(rc)
        else:
            means, counts = fcd.convergence_depths(m["d"], m["m"], counts=True)

        def check():
            got = means.cpu().numpy()
            bad = cr.same_bits(got, m["want"])
            assert bad.size == 0, f"convergence depths ({through}): frames {bad.tolist()} differ: got {got.tolist()} want {m['want'].tolist()}"
            assert counts.cpu().numpy().tolist() == m["counts"].tolist(), f"convergence counts ({through}) differ"
        return check


def overlaps(logs):
    """{family: pairs of steps of different threads, one of them of that family, whose [t_enter, t_exit] intersect}."""
    entries = [e for log in logs for e in log]
    pairs = {fam: 0 for fam in FAMILIES}
    for i, (ta, _sa, fa, a0, a1) in enumerate(entries):
        for tb, _sb, fb, b0, b1 in entries[i + 1:]:
            if ta != tb and a0 < b1 and b0 < a1:
                pairs[fa] += 1
                if fb != fa:
                    pairs[fb] += 1
    return pairs


def run_in_threads(workers, limit, extra=()):
    """Starts one daemon thread per worker (and per callable of `extra`), joins them within `limit` seconds in all -> the names of
    the threads still alive (then nothing more may be started on the GPU)."""
    threads = [threading.Thread(target=w.run, name=f"worker-{w.index}", daemon=True) for w in workers]
    threads += [threading.Thread(target=fn, name=fn.__name__, daemon=True) for fn in extra]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, limit - (time.perf_counter() - t0)))
    return [t.name for t in threads if t.is_alive()]
