"""One render context kept across many calls, configurations and streams, as clip.py keeps one for a whole clip -- every output
bit for bit against the oracle for the configuration in force at that call.

The C ABI lets a caller change a live context's configuration at any time (mdvt_set_config, mdvt_set_near_clip), while the
context carries state from call to call: the cached parameter block, the division-check table, the z-key slot parities, the
scanline -> cell table of the sub-pixel grid, workspace sized by frames and by the planes a configuration needs, the hole-count
buffers, the multisample and near-clip key planes, the banks' side stream, and the workspaces of the completion, the normal
infill and the FFV1 encoder.  The other GPU tests mostly build a fresh context per configuration; here one context lives through:

1. seeded random walks (test_random_walk_on_one_context): reconfigure, render a batch of mixed frames, run an entry point that
   shares the workspace.  A failure names the walk seed, the step, the configuration and the steps before it.
   MDVT_SWEEP_SEED changes the walks, MDVT_REUSE_STEPS (default 1) multiplies their steps for soaks;
2. more parameter sets than the division-check table holds (the fast point kernel's IEEE branch);
3. one context used from three streams, new parameter sets brought in on side streams;
4. two contexts created and closed in the middle of each other's work (pooled workspace blocks change hands);
5. the regressions the walks found, each under its own name.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MDVT_ERR_UNSUPPORTED = -3
GREEN, BLACK = (0, 255, 0), (0, 0, 0)


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from metric_depth_video_toolbox_amd import _lib, stereo_rerender, synthetic
    return _lib, stereo_rerender, synthetic


def _K(p):
    return np.array([p.K[k] for k in range(9)]).reshape(3, 3)


def _default_bits():
    return int(os.environ.get("MDVT_TEST_SUBPIXEL_BITS", "0") or 0)


# ------------------------------------------------------------------------------------------------ configuration of a live context
def base_cfg(**kw):
    cfg = dict(mesh=True, rm=False, ep=0, key=BLACK, cull=0, bits=_default_bits(), samples=0, pattern=0, resolve=0, near_clip=0,
               ipd=65, max_depth=100, ws_mib=0)
    cfg.update(kw)
    return cfg


def apply_cfg(_lib, r, cfg):
    """mdvt_set_config + mdvt_set_near_clip on the live context, and the renderer's Python-side fields kept in step (render() sizes
    and allows outputs from them, frame_params() takes the ipd from them, finish_infill_mask_sbs's second context follows _cfg)."""
    L = _lib.load()
    c = _lib.MdvtConfig()
    c.mode = _lib.MODE_MESH if cfg["mesh"] else _lib.MODE_POINTS
    c.remove_edges, c.edge_points, c.cull = int(cfg["rm"]), int(cfg["ep"]), int(cfg["cull"])
    c.workspace_mib, c.subpixel_bits = int(cfg["ws_mib"]), int(cfg["bits"])
    c.samples, c.sample_pattern, c.sample_resolve = int(cfg["samples"]), int(cfg["pattern"]), int(cfg["resolve"])
    c.ipd_m, c.max_depth = cfg["ipd"] / 1000, float(cfg["max_depth"])
    for k in range(3):
        c.key_rgb[k] = cfg["key"][k]
    r.ctx.check(L.mdvt_set_config(r.ctx.handle, C.byref(c)))
    r.ctx.check(L.mdvt_set_near_clip(r.ctx.handle, int(cfg["near_clip"])))
    r.mode = c.mode
    r.remove_edges, r.edge_points, r.do_basic_infill = bool(cfg["rm"]), cfg["ep"] != 0, cfg["ep"] == 2
    r.key_rgb, r.cull, r.subpixel_bits = tuple(cfg["key"]), int(cfg["cull"]), int(cfg["bits"])
    r.samples, r.sample_pattern, r.sample_resolve = int(cfg["samples"]), int(cfg["pattern"]), int(cfg["resolve"])
    r.near_clip = bool(cfg["near_clip"])
    r.pupillary_distance, r.max_depth = cfg["ipd"], cfg["max_depth"]
    r._cfg = c


def gl_path(cfg):
    """The call renders on the multisample or the near-clip path (the GL candidate of the oracle is its reference)."""
    return cfg["samples"] == 4 or (cfg["near_clip"] and cfg["mesh"])


def oracle_frame(orc, W, H, cfg, p, T, d, c, want_depth=False, want_seed=False):
    op = orc.make_params(W, H, _K(p), ipd_m=cfg["ipd"] / 1000, max_depth=cfg["max_depth"], depth_scale=p.depth_scale,
                         mode=orc.MODE_MESH if cfg["mesh"] else orc.MODE_POINTS, remove_edges=cfg["rm"],
                         edge_points=0 if gl_path(cfg) else int(cfg["ep"]), conv_angle=p.convergence_angle, T=T, key_rgb=cfg["key"],
                         cull=cfg["cull"], subpixel_bits=cfg["bits"])
    if gl_path(cfg):
        return orc.render_stereo_gl(op, d, c, near_clip=bool(cfg["near_clip"] and cfg["mesh"]),
                                    samples=4 if cfg["samples"] == 4 else 1, pattern=cfg["pattern"], resolve=cfg["resolve"])
    return orc.render_stereo(op, d, c, want_depth=want_depth, want_seed=want_seed)


def check_frame(got, f, want, W, tag):
    """Every plane the call asked for, frame f, against the oracle's frame."""
    sbs, mask = got["sbs"][f].cpu().numpy(), got["mask"][f].cpu().numpy() if "mask" in got else None
    for e, (eye, sl) in enumerate((("left", slice(0, W)), ("right", slice(W, 2 * W)))):
        wm = want[eye + "_mask"]
        if mask is not None:
            assert np.array_equal(mask[:, sl], wm), f"{tag}: {eye} mask differs at {int((mask[:, sl] != wm).sum())} px"
        assert np.array_equal(sbs[:, sl], want[eye + "_rgb"]), \
            f"{tag}: {eye} rgb differs at {int(np.any(sbs[:, sl] != want[eye + '_rgb'], -1).sum())} px"
        if "depth" in got:
            z = got["depth"][f].cpu().numpy()[:, sl]
            assert np.array_equal(z.view(np.uint32), want[eye + "_depth"].view(np.uint32)), f"{tag}: {eye} depth plane differs"
        if "seed" in got:
            assert np.array_equal(got["seed"][f].cpu().numpy()[:, sl], want[eye + "_seed"]), f"{tag}: {eye} seed image differs"
        if "maskbits" in got:
            wb = np.packbits(wm > 0, axis=1, bitorder="little")
            assert np.array_equal(got["maskbits"][f, :, e, :wb.shape[1]].cpu().numpy(), wb), f"{tag}: {eye} packed mask differs"
        if "hole_counts" in got:
            assert int(got["hole_counts"][f, e]) == int((wm > 0).sum()), f"{tag}: {eye} hole count differs"


# ------------------------------------------------------------------------------------------------ inputs
def depth_code_rgb(code):
    code = np.minimum(np.asarray(code, np.int64), 65535).astype(np.uint32)
    d = np.zeros(code.shape + (3,), np.uint8)
    d[..., 0] = (code >> 8) & 0xFF
    d[..., 1] = d[..., 0]
    d[..., 2] = code & 0xFF
    return d


def frame_pool(synthetic, W, H, rng, n=6):
    """Synthetic scenes with depth-code-0 patches and exact key colours, and a few cheap depth styles of the batch sweep."""
    ds, cs = [], []
    for k in range(n):
        if k % 3 == 2:
            style = int(rng.integers(3))
            if style == 0:
                code = np.full((H, W), int(rng.integers(3000, 60000)))
                for _ in range(int(rng.integers(1, 5))):
                    x0, y0 = int(rng.integers(W)), int(rng.integers(H))
                    code[y0:y0 + int(rng.integers(1, H + 1)), x0:x0 + int(rng.integers(1, W + 1))] = int(rng.integers(50, 3000))
            elif style == 1:
                code = int(rng.integers(300, 40000)) + np.arange(W)[None, :] // 3 + rng.integers(0, 2, (H, W))
            else:
                near, far = int(rng.integers(20, 400)), int(rng.integers(5000, 65000))
                stripes = np.broadcast_to((np.arange(W)[None, :] if rng.integers(2) else np.arange(H)[:, None]) // int(rng.integers(1, 4)) % 2, (H, W))
                code = np.where(stripes == 0, near, far)
            d = depth_code_rgb(code)
            c = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        else:
            d, c = synthetic.SyntheticScene(W, H, seed=int(rng.integers(1 << 30)), n_fg=6).frame(int(rng.integers(0, 50)))
        if H > 8 and W > 16:
            h, w = max(2, H // 10), max(4, W // 10)
            y0, x0 = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
            d[y0:y0 + h, x0:x0 + w] = 0                              # Z = 0: behind the near plane
            c[1, 2], c[2, 7], c[H // 2, W // 2] = BLACK, GREEN, BLACK   # exact key colours
        ds.append(np.ascontiguousarray(d)); cs.append(np.ascontiguousarray(c))
    return np.stack(ds), np.stack(cs)


KIND_NAMES = ("pure", "conv", "pose", "both")


def frame_params(r, synthetic, rng, kind, xfov):
    T = synthetic.synthetic_pose_track(64)[int(rng.integers(1, 64))] if kind in (2, 3) else None
    conv = float(rng.uniform(0.8, 8.0)) if kind in (1, 3) else None
    return r.frame_params(xfov=xfov, convergence_distance=conv, transformation=T), T


def synthetic_seed(rng, W, H, key):
    """An infill-mask seed: key-coloured holes with normal-coloured points along their edges on black."""
    seed = np.zeros((H, W, 3), np.uint8)
    for _ in range(4):
        x0, y0 = int(rng.integers(0, max(1, W - 3))), int(rng.integers(0, max(1, H - 3)))
        w, h = int(rng.integers(2, max(3, W // 3))), int(rng.integers(2, max(3, H // 2)))
        seed[y0:y0 + h, x0:x0 + w] = key if key != BLACK else (0, 0, 0)
        for _ in range(w + h):
            seed[min(H - 1, y0 + int(rng.integers(0, h))), min(W - 1, x0 + int(rng.integers(0, 2)))] = rng.integers(1, 255, 3)
    seed[0, :] = np.where(np.all(seed[0, :] == 0, -1)[:, None], np.array([255, 127, 127], np.uint8), seed[0, :])
    return seed


def fmm_finish(orc, seed, key):
    """sr:803-808 in cv2.inpaint's own order (as tests/test_gpu_inpaint_heap.py)."""
    keym = np.all(seed == np.array(key, np.uint8), -1)
    mask = (keym | np.all(seed == 0, -1)).astype(np.uint8)
    filled = orc.telea_fmm(seed, mask)
    merged = seed.copy()
    merged[keym] = filled[keym]
    return orc.masked_blur(merged)


def ni_inputs(rng, img):
    """normal_infill's inputs from a colour image: a normal-coloured infill mask over a few blobs, the image black under it."""
    H, W = img.shape[:2]
    img = img.copy()
    mask = np.zeros((H, W, 3), np.uint8)
    for _ in range(3):
        x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        w, h = int(rng.integers(1, max(2, W // 4))), int(rng.integers(1, max(2, H // 3)))
        ang = rng.uniform(0, 2 * np.pi)
        mask[y0:y0 + h, x0:x0 + w] = ((np.cos(ang) + 1) / 2 * 255, (np.sin(ang) + 1) / 2 * 255, rng.uniform(40, 255))
    img[np.any(mask != 0, -1)] = 0
    return img, mask


# ------------------------------------------------------------------------------------------------ the walk
def random_cfg(rng, prev, W, H):
    """prev with one to four fields changed (a new context's first configuration when prev is None)."""
    cfg = dict(prev) if prev is not None else base_cfg()
    fields = ["mesh", "rm", "ep", "key", "cull", "bits", "samples", "near_clip", "ipd", "max_depth", "ws_mib"]
    for f in (fields if prev is None else rng.choice(fields, int(rng.integers(1, 5)), replace=False)):
        if f == "mesh": cfg["mesh"] = bool(rng.integers(4) != 0)
        elif f == "rm": cfg["rm"] = bool(rng.integers(2))
        elif f == "ep": cfg["ep"] = int(rng.integers(3))
        elif f == "key": cfg["key"] = GREEN if rng.integers(2) else BLACK
        elif f == "cull": cfg["cull"] = int(rng.integers(3))
        elif f == "bits": cfg["bits"] = int(rng.choice([0, 4, 8]))
        elif f == "samples":
            cfg["samples"] = 4 if rng.integers(4) == 0 else int(rng.integers(2))
            cfg["pattern"], cfg["resolve"] = int(rng.integers(2)), int(rng.integers(2))
        elif f == "near_clip": cfg["near_clip"] = int(rng.integers(4) == 0)
        elif f == "ipd": cfg["ipd"] = int(rng.choice([1, 30, 63, 65, 120]))
        elif f == "max_depth": cfg["max_depth"] = int(rng.choice([20, 100, 655]))
        elif f == "ws_mib":
            # the library's default, or a budget of 2 ... 6 slots of the posed / converged mesh path (launch sets on two banks).
            # (workspace_mib counts whole MiB, rounded up here: the budget affords at least `slots` slots.  Below about 700 px one
            #  MiB already affords more than the 16 slots a launch set takes at most, so at 33 x 17 the budget changes nothing and
            #  the banks are reached by the larger walks only)
            slots = int(rng.choice([0, 2, 3, 4, 6]))
            per_slot = W * H * (16 + 16 + 32 + 28 + 3)
            cfg["ws_mib"] = 0 if slots == 0 else max(1, -(-slots * per_slot // (1 << 20)))
    if prev is None and _default_bits():
        cfg["bits"] = _default_bits()   # (MDVT_TEST_SUBPIXEL_BITS: the walk starts on that grid; later steps switch among 0 / 4 / 8)
    if not cfg["rm"]:
        cfg["ep"] = 0
    if gl_path(cfg) and rng.integers(6) != 0:
        cfg["ep"] = 0                  # (mostly: the multisample / near-clip paths refuse edge points -- and sometimes the walk asks)
    return cfg


def cfg_str(cfg):
    return ("mesh" if cfg["mesh"] else "points") + "".join(
        f" {k}={v}" for k, v in cfg.items() if k != "mesh" and (k not in ("pattern", "resolve") or cfg["samples"] == 4))


WALKS = [(33, 17, 200, 24), (160, 90, 120, 24), (250, 61, 80, 16), (640, 480, 16, 3)]      # W, H, steps, most frames per call


class Walker:
    """One context of a random walk: step() reconfigures (mostly), renders a batch of mixed frames against the oracle and runs one
    of the entry points that share the context's workspace."""

    def __init__(self, mods, orc, W, H, max_frames, seed):
        _lib, sr, synthetic = mods
        self.mods, self.orc, self.W, self.H, self.max_frames, self.seed = mods, orc, W, H, max_frames, seed
        self.rng = np.random.default_rng(seed)
        self.depth, self.color = frame_pool(synthetic, W, H, self.rng)
        self.d_all, self.c_all = torch.from_numpy(self.depth).cuda(), torch.from_numpy(self.color).cuda()
        self.r = sr.StereoRerenderer(W, H, pupillary_distance=65)
        self.cfg, self.history = None, []

    def close(self):
        torch.cuda.synchronize()
        self.r.close()

    def step(self, step):
        _lib, _, synthetic = self.mods
        from metric_depth_video_toolbox_amd import ffv1_device, video_io
        orc, W, H, max_frames, seed, rng, r = self.orc, self.W, self.H, self.max_frames, self.seed, self.rng, self.r
        depth, color, d_all, c_all, history, cfg = self.depth, self.color, self.d_all, self.c_all, self.history, self.cfg
        if cfg is None or rng.integers(3) != 0:
            cfg = self.cfg = random_cfg(rng, cfg, W, H)
            apply_cfg(_lib, r, cfg)
        history.append(f"step {step}: {cfg_str(cfg)}")
        tag0 = f"walk seed={seed} {W}x{H} step {step} [{cfg_str(cfg)}]; before: " + " | ".join(history[-4:-1])
        # ---- render a batch of mixed frames
        N = int(rng.integers(1, max_frames + 1))
        idx = rng.integers(0, len(depth), N)
        layout = int(rng.integers(3))
        base = int(rng.integers(4))
        kinds = [base if layout == 0 else int(rng.integers(4)) if layout == 1 else (base if f < N // 2 else (base + 1) % 4)
                 for f in range(N)]
        xfov = float(rng.choice([45.0, 60.0, 90.0]))
        pts = [frame_params(r, synthetic, rng, k, xfov) for k in kinds]
        ps, Ts = [p for p, _ in pts], [T for _, T in pts]
        d, c = d_all[torch.from_numpy(idx).cuda()].contiguous(), c_all[torch.from_numpy(idx).cuda()].contiguous()
        gl = gl_path(cfg)
        want = dict(want_hole_counts=bool(rng.integers(2)))
        if not gl:
            want.update(want_depth=bool(rng.integers(2)), want_maskbits=bool(rng.integers(3) == 0),
                        want_seed=cfg["rm"] and bool(rng.integers(2)))
        tag = f"{tag0}; render {N} frames kinds={''.join(KIND_NAMES[k][0] for k in kinds)} xfov={xfov} outputs={want}"
        if gl and (cfg["ep"] or rng.integers(5) == 0):
            # a refused output (or a configuration that refuses edge points): the documented code, and the next call is exact
            refusable = ["want_depth", "want_maskbits"] + (["want_seed"] if cfg["rm"] else [])
            bad = {} if cfg["ep"] else {refusable[int(rng.integers(len(refusable)))]: True}
            with pytest.raises(_lib.MdvtError) as e:
                r.render(d, c, ps, **want, **bad)
            assert e.value.code == MDVT_ERR_UNSUPPORTED, f"{tag}: refusal of {bad or 'edge points'} gave {e.value.code}"
            history[-1] += f" refused {bad or 'edge points'}"
            if cfg["ep"]:
                return
        got = r.render(d, c, ps, **want)
        history[-1] += f" N={N} kinds={''.join(KIND_NAMES[k][0] for k in kinds)} {sorted(k for k, v in want.items() if v)}"
        for f in range(N):
            wf = oracle_frame(orc, W, H, cfg, ps[f], Ts[f], depth[idx[f]], color[idx[f]], want_depth=want.get("want_depth", False),
                              want_seed=want.get("want_seed", False))
            check_frame(got, f, wf, W, f"{tag}, frame {f} ({KIND_NAMES[kinds[f]]}, pool {idx[f]})")
        # ---- an entry point that shares the context's workspace
        aux = str(rng.choice(["none", "finish", "heap", "finish_sbs", "normal_infill", "mask_normals", "edge_filter", "ffv1"],
                             p=[0.3, 0.12, 0.08, 0.1, 0.1, 0.1, 0.1, 0.1]))
        history[-1] += f" + {aux}"
        tag = f"{tag0}; {aux} after the render"
        key = tuple(cfg["key"])
        if aux in ("finish", "heap", "finish_sbs"):
            if "seed" in got:
                seeds = got["seed"][:, :, :W]                               # left eyes: a strided view of the side-by-side seeds
            else:
                seeds = torch.from_numpy(np.stack([synthetic_seed(rng, W, H, key) for _ in range(min(N, 3))])).cuda()
            seeds_np = seeds.cpu().numpy()
            if aux == "finish":
                out, rem = r.finish_infill_mask(seeds, max_rounds=W + H, want_remaining=True)
                for k in range(len(seeds_np)):
                    wimg, wrem = orc.finish_infill_mask(seeds_np[k], key_rgb=key, max_rounds=W + H)
                    assert np.array_equal(out[k].cpu().numpy(), wimg), f"{tag}: image {k} differs"
                    assert int(rem[k]) == wrem, f"{tag}: image {k} remaining {int(rem[k])} != {wrem}"
            elif aux == "heap":
                out = r.finish_infill_mask(seeds, order="heap")
                for k in range(len(seeds_np)):
                    assert np.array_equal(out[k].cpu().numpy(), fmm_finish(orc, seeds_np[k], key)), f"{tag}: image {k} differs"
            else:
                # 32 frames: two halves on two contexts (StereoRerenderer.FINISH_SPLIT_FRAMES) -- the second follows the first's
                # configuration as it is now
                n = len(seeds_np)
                pick = rng.integers(0, n, (32, 2))
                sbs = torch.cat([seeds[torch.from_numpy(pick[:, 0]).cuda()], seeds[torch.from_numpy(pick[:, 1]).cuda()]], dim=2).contiguous()
                out, rem = r.finish_infill_mask_sbs(sbs, max_rounds=W + H, want_remaining=True)
                wants = [orc.finish_infill_mask(seeds_np[k], key_rgb=key, max_rounds=W + H) for k in range(n)]
                out = out.cpu().numpy()
                for f in range(32):
                    for e in range(2):
                        wimg, wrem = wants[pick[f, e]]
                        assert np.array_equal(out[f, :, e * W:(e + 1) * W], wimg), f"{tag}: frame {f} eye {e} differs"
                        assert int(rem[e, f]) == wrem, f"{tag}: frame {f} eye {e} remaining differs"
        elif aux in ("normal_infill", "mask_normals"):
            img, mask = ni_inputs(rng, got["sbs"][0, :, :W].cpu().numpy())
            d_img, d_mask = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()
            L = _lib.load()
            s = torch.cuda.current_stream()
            if aux == "normal_infill":
                out = torch.empty_like(d_img)
                r.ctx.check(L.mdvt_normal_infill(r.ctx.handle, d_img.data_ptr(), 3 * W, 0, d_mask.data_ptr(), 3 * W, 0,
                                                 out.data_ptr(), 3 * W, 0, 1, C.c_void_p(s.cuda_stream)))
                assert np.array_equal(out.cpu().numpy(), orc.normal_infill(img, mask)), tag
            else:
                hole = np.any(mask != 0, -1)
                d_hole = torch.from_numpy(hole.astype(np.uint8) * 255).cuda()
                r.ctx.check(L.mdvt_infill_using_mask_normals(r.ctx.handle, d_img.data_ptr(), 3 * W, 0, d_hole.data_ptr(), W, 0,
                                                             d_mask.data_ptr(), 3 * W, 0, 1, 400, C.c_void_p(s.cuda_stream)))
                wn = ((mask.astype(np.float32) / np.float32(255.0)) * 2 - 1).astype(np.float32)
                assert np.array_equal(d_img.cpu().numpy(), orc.infill_using_normals(img, hole, wn)), tag
        elif aux == "edge_filter":
            k = int(rng.integers(N))
            tri, unused = r.edge_filter(d[k], ps[k])
            zs = orc.decode_depth(depth[idx[k]], cfg["max_depth"], ps[k].depth_scale)
            wt, wu, _ = orc.edge_filter(zs, _K(ps[k]), cfg["mesh"])
            assert np.array_equal(tri.cpu().numpy(), wt) and np.array_equal(unused.cpu().numpy(), wu), tag
        elif aux == "ffv1":
            slices = ((1, 1), (2, 2), (4, 2))[int(rng.integers(3))]
            pk = ffv1_device.enqueue(r.ctx, got["sbs"], slices=slices).collect()
            host = got["sbs"].cpu().numpy()
            for f in range(N):
                assert pk[f] == video_io.encode_frame(host[f], slices=slices)[0], f"{tag}: frame {f} packet differs"


def walk(mods, orc, W, H, steps, max_frames, seed):
    w = Walker(mods, orc, W, H, max_frames, seed)
    try:
        for step in range(steps):
            w.step(step)
    finally:
        w.close()


def walk_cases():
    seed0 = int(os.environ.get("MDVT_SWEEP_SEED", "20261016"))
    mult = float(os.environ.get("MDVT_REUSE_STEPS", "1"))
    return [(W, H, max(1, int(round(steps * mult))), nf, seed0 + 1000 * i) for i, (W, H, steps, nf) in enumerate(WALKS)]


@pytest.mark.parametrize("W,H,steps,max_frames,seed", walk_cases(), ids=lambda v: str(v))
def test_random_walk_on_one_context(mods, orc, W, H, steps, max_frames, seed):
    walk(mods, orc, W, H, steps, max_frames, seed)



# ------------------------------------------------------------------------------------------------ 2. the division-check table overflows
def _all_codes(rng):
    """256 x 256 frames holding every one of the 65 536 depth codes (code = row * 256 + col), random colour."""
    return depth_code_rgb(np.arange(65536).reshape(256, 256)), rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)


def boundary_frame(p, cfg, bits, W, H):
    """Depth codes placed where the disparity's last bit decides the column: the pure-shift point column is
    (rint(S (j +- d)) - 1) >> log2 S with d = dl / z in f32, so a code whose d sits within a few ulps of k +- 1 / (2 S) flips the
    column of some j when d is off by one ulp.  Such (code, j) pairs for this frame's parameter set, one per row (the rest of the
    row code 0: no point), so that nothing covers them -- a division wrong in its last bit moves a point and the frame differs.
    -> (depth_rgb, pairs placed)."""
    S = np.float32(1 << bits)
    mult, scale = np.float32(cfg["max_depth"] / 4228250625.0), np.float32(p.depth_scale)      # (fill_frame_dev's operands)
    dl = np.float32(p.Krender[0] * ((cfg["ipd"] / 1000) / 2.0))
    codes = np.arange(1, 65536, dtype=np.uint32)
    z = ((codes << 16).astype(np.float32) * mult) * scale
    d = dl / z
    h = np.float32(0.5) / S
    near = (z > np.float32(1e-4)) & ((np.abs(d - (np.rint(d - h) + h)) < 2.0 ** -11) | (np.abs(d - (np.rint(d + h) - h)) < 2.0 ** -11))
    j = np.arange(W, dtype=np.float32)
    hits = []
    for code, dv in zip(codes[near], d[near]):
        for sgn in (1, -1):
            cols = [(np.rint((j + x if sgn > 0 else j - x) * S).astype(np.int64) - 1) >> bits
                    for x in (dv, np.nextafter(dv, np.float32(np.inf)), np.nextafter(dv, np.float32(0)))]
            flip = ((cols[0] != cols[1]) | (cols[0] != cols[2])) & (((cols[0] >= 0) & (cols[0] < W)) | ((cols[1] >= 0) & (cols[1] < W)))
            hits += [(int(code), int(jj)) for jj in np.nonzero(flip)[0]]
    plane = np.zeros((H, W), np.int64)
    for r, (code, jj) in enumerate(hits[:H]):
        plane[r, jj] = code
    return depth_code_rgb(plane), min(len(hits), H)


def test_more_parameter_sets_than_the_division_table_holds(mods, orc):
    """k_points_rows_fast takes the proven short division for a parameter set (mult, scale, dl) with a slot in the context's table
    of division checks (256 slots) and the IEEE division dl / z otherwise.  ~300 distinct (xfov, ipd, max_depth) sets on one
    points context, in batches that straddle set 256, with and without the packed mask and hole counts (and the byte mask left
    out); then early sets again (slot lookup) and new ones (the IEEE branch).  Every depth code is in every other frame; the frames
    between them hold the codes whose column a one-ulp error in that frame's division would move (boundary_frame)."""
    _lib, sr, synthetic = mods
    W = H = 256
    rng = np.random.default_rng(256)
    d0, c0 = _all_codes(rng)
    colors = np.stack([c0] + [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2)])
    r = sr.StereoRerenderer(W, H, render_as_pointcloud=True)
    try:
        cfg = base_cfg(mesh=False, bits=r.subpixel_bits)
        combos = [(ipd, md) for ipd in (55, 63, 65, 70) for md in (20, 100, 655)]
        bits = 4 if r.subpixel_bits == 4 else 8
        seen, placed = [], []

        def batch(b, xfovs, ipd, md):
            cfg.update(ipd=ipd, max_depth=md)
            apply_cfg(_lib, r, cfg)
            n = len(xfovs)
            ci = rng.integers(0, len(colors), n)
            c = torch.from_numpy(colors[ci]).cuda()
            ps = [r.frame_params(xfov=x) for x in xfovs]
            assert all(p.has_T == 0 and p.convergence_angle == 0.0 for p in ps)
            ds = []
            for f in range(n):
                if f == 0 or (f % 2 == 0 and b < 36):                # (from set 252 on, mostly the frames that test the last bit)
                    ds.append(d0)
                else:
                    bf, k = boundary_frame(ps[f], cfg, bits, W, H)
                    ds.append(bf)
                    placed.append(k)
            d = torch.from_numpy(np.stack(ds)).cuda()
            out = [dict(), dict(want_maskbits=True, want_hole_counts=True), dict(want_maskbits=True, want_hole_counts=True, want_mask=False),
                   dict(want_depth=True)][b % 4]
            got = r.render(d, c, ps, **out)
            for f in range(n):
                want = oracle_frame(orc, W, H, cfg, ps[f], None, ds[f], colors[ci[f]], want_depth="want_depth" in out)
                check_frame(got, f, want, W, f"batch {b} frame {f}: xfov={xfovs[f]} ipd={ipd} max_depth={md} outputs={out}")

        k = 0
        for b in range(43):                                           # 301 sets: set 256 is the fifth frame of batch 36
            ipd, md = combos[b % len(combos)]
            xfovs = [35.0 + 0.173 * (k + i) for i in range(7)]
            k += 7
            batch(b, xfovs, ipd, md)
            seen.append((xfovs, ipd, md))
        for b, (xfovs, ipd, md) in enumerate(seen[:5] + seen[34:38]):     # sets with a slot, then sets without one
            batch(100 + b, xfovs, ipd, md)
        for b in range(4):                                            # new sets: the table stays full, they take the IEEE division
            batch(200 + b, [110.0 + 0.31 * (7 * b + i) for i in range(7)], *combos[b])
        assert sum(placed) > 400, f"only {sum(placed)} column-deciding depth codes placed"
    finally:
        torch.cuda.synchronize()
        r.close()


# ------------------------------------------------------------------------------------------------ 3. one context on three streams
def test_one_context_on_three_streams(mods, orc):
    """Pure-shift point renders without hole counts use no workspace of the context: byte masks, packed mask bits and depth planes
    go straight to the caller's buffers, so the caller's buffer contract asks for no ordering between such calls on different
    streams.  Hole counts go through the context's per-wave count buffers (mdvt.h: one stream at a time), so the calls that ask
    for them all stay on the current stream, which orders them among themselves.  One context alternates between the current
    stream and two side streams with no host synchronisation; new parameter sets come in on a side stream first and are used next
    on another stream (their division check has to be ordered before those renders).  Outputs compared after the final
    synchronisation.  (No test can force the race this guards against: the outputs only change where the short division would be
    wrong for unproven operands.)"""
    _lib, sr, synthetic = mods
    W, H = 256, 96
    rng = np.random.default_rng(3)
    r = sr.StereoRerenderer(W, H, render_as_pointcloud=True)
    try:
        cfg = base_cfg(mesh=False, bits=r.subpixel_bits)
        apply_cfg(_lib, r, cfg)
        depth, color = frame_pool(synthetic, W, H, rng, n=4)
        d_all, c_all = torch.from_numpy(depth).cuda(), torch.from_numpy(color).cuda()
        cur = torch.cuda.current_stream()
        side = [torch.cuda.Stream(), torch.cuda.Stream()]
        plan, jobs = [], []
        introduced = []
        for call in range(30):
            st = (1, 2, 0, 2, 0, 1)[call % 6]                     # 0: the current stream
            if st and (not introduced or rng.integers(3) != 0):
                introduced.append(40.0 + 0.7 * len(introduced))    # a new set, first seen on a side stream
            n = int(rng.integers(1, 5))
            xf = [introduced[-1] if (st and f == 0) else float(rng.choice(introduced)) for f in range(n)]
            idx = rng.integers(0, len(depth), n)
            ps = [r.frame_params(xfov=x) for x in xf]
            kw = [dict(), dict(want_depth=True), dict(want_maskbits=True), dict(want_maskbits=True, want_mask=False)][call % 4]
            if st == 0 and call % 3 == 2:
                kw = dict(kw, want_hole_counts=True)              # (the context's count buffers: only ever on this one stream)
            jobs.append(r.prepare(d_all[torch.from_numpy(idx).cuda()].contiguous(), c_all[torch.from_numpy(idx).cuda()].contiguous(),
                                  ps, **kw))
            plan.append((st, xf, idx, ps, kw))
        assert any("want_hole_counts" in kw for *_x, kw in plan)
        for s in side:
            s.wait_stream(cur)                                    # inputs gathered, outputs allocated and zeroed on the current stream
        for job, (st, *_rest) in zip(jobs, plan):
            job.launch(cur if st == 0 else side[st - 1])
        torch.cuda.synchronize()
        for call, (job, (st, xf, idx, ps, kw)) in enumerate(zip(jobs, plan)):
            for f in range(len(xf)):
                want = oracle_frame(orc, W, H, cfg, ps[f], None, depth[idx[f]], color[idx[f]], want_depth="want_depth" in kw)
                check_frame(job.results, f, want, W, f"call {call} on stream {st}, frame {f} xfov={xf[f]} {kw}")
    finally:
        torch.cuda.synchronize()
        r.close()


# ------------------------------------------------------------------------------------------------ 4. two contexts, interleaved
def test_two_contexts_interleaved_across_create_and_close(mods, orc):
    """Two walks of the same frame size take turns on one GPU; every few steps one context is closed and a fresh one made in its
    place, so workspace blocks go back to the library's pool and come out again in the other context (or the new one)."""
    seed0 = int(os.environ.get("MDVT_SWEEP_SEED", "20261016")) + 77
    W, H = 96, 64
    walkers = [Walker(mods, orc, W, H, 12, seed0), Walker(mods, orc, W, H, 12, seed0 + 1)]
    made = 2
    try:
        for step in range(int(round(60 * float(os.environ.get("MDVT_REUSE_STEPS", "1"))))):
            k = step % 2
            if step % 5 == 4:
                walkers[k].close()
                walkers[k] = Walker(mods, orc, W, H, 12, seed0 + made)
                made += 1
            walkers[k].step(step)
    finally:
        for w in walkers:
            w.close()


# ------------------------------------------------------------------------------------------------ 5. regressions
def test_finish_in_two_halves_follows_a_reconfigured_key(mods, orc):
    """finish_infill_mask_sbs from 32 frames runs its second half on a second context, made on first use.  It has to take the
    first context's configuration as it is at the call (the key colour decides what is filled), not as it was when made.
    Found by the walks: with the second context left at its first configuration, three of the four fail at their first
    32-frame completion after a key change."""
    _lib, sr, synthetic = mods
    W, H = 64, 40
    rng = np.random.default_rng(41)
    r = sr.StereoRerenderer(W, H, infill_mask=True)
    try:
        cfg = base_cfg(rm=True, ep=1, key=GREEN, bits=r.subpixel_bits)
        for key in (GREEN, BLACK, GREEN):
            cfg["key"] = key
            apply_cfg(_lib, r, cfg)
            seeds = np.stack([synthetic_seed(rng, W, H, key) for _ in range(2)])
            sbs = np.ascontiguousarray(np.broadcast_to(np.concatenate([seeds[0], seeds[1]], 1), (32, H, 2 * W, 3)))
            out, rem = r.finish_infill_mask_sbs(torch.from_numpy(sbs).cuda(), max_rounds=W + H, want_remaining=True)
            out = out.cpu().numpy()
            for e in range(2):
                wimg, wrem = orc.finish_infill_mask(seeds[e], key_rgb=key, max_rounds=W + H)
                for f in (0, 31):
                    assert np.array_equal(out[f, :, e * W:(e + 1) * W], wimg), (key, f, e)
                    assert int(rem[e, f]) == wrem, (key, f, e)
    finally:
        torch.cuda.synchronize()
        r.close()
