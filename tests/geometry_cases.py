"""What the GPU tests of the geometry export share: depth frames with the features a case needs, one raw call of
mdvt_export_geometry_batch on poisoned buffers, and the comparison of everything it wrote -- and left alone -- with
tests/geometry_ref.py.  TEST INFRASTRUCTURE ONLY: plain module, no fixture, no pytest setting."""
import ctypes as C

import numpy as np

import geometry_ref as gr

OUTPUTS = ("vertices", "triangles", "used_index", "points", "point_rgb")
POISON = 0xA5
ITEM = {"vertices": 24, "triangles": 12, "used_index": 4, "points": 24, "point_rgb": 3}          # bytes per entry
DTYPE = {"vertices": np.float64, "triangles": np.int32, "used_index": np.int32, "points": np.float64, "point_rgb": np.uint8}
# the compaction's spans (csrc/mdvt_internal.h): a workgroup counts and scatters kGeomBlock = 256 items of a list, one step of the
# scan takes kGeomScan = 256 workgroup totals, i.e. 65 536 items
GEOM_BLOCK, GEOM_SCAN = 256, 256


def K_of(W, H, xfov=60.0):
    fx = W / (2 * np.tan(np.deg2rad(xfov) / 2))
    return np.array([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]], np.float64)


def code_frame(code, split=False):
    """uint16 codes [H, W] -> RGB-coded depth.  split: G = R ^ 1, an odd R + G whose halved sum decode 0 takes for the high byte."""
    code = np.asarray(code).astype(np.int64) & 0xFFFF
    out = np.empty(code.shape + (3,), np.uint8)
    out[..., 0] = out[..., 1] = code >> 8
    out[..., 2] = code & 0xFF
    if split:
        out[..., 1] ^= 1
    return out


def scene(rng, H, W, f=0, split=False):
    """A tilted background, a near box with a depth step at its rim (triangles for the 89-degree filter), noise in the low byte, a
    few pixels of depth code 0."""
    y, x = np.mgrid[0:H, 0:W]
    code = (9000 + 40 * x + 25 * y + 700 * f).astype(np.int64)
    x0, y0 = (W // 4 + f) % max(W - 2, 1), (H // 3 + f) % max(H - 1, 1)
    code[y0:y0 + max(H // 3, 1), x0:x0 + max(W // 3, 1)] = 1500 + 100 * f
    code = (code + rng.integers(0, 64, (H, W))) & 0xFFFF
    code[rng.random((H, W)) < 0.02] = 0
    if W * H > 4:
        code[0, 0] = 0
    return code_frame(code, split)


def stripes(rng, H, W):
    """Columns far, far, far, near, ...: the cells on both sides of every near column are removed, its vertices (inner rows) unused,
    the cells between far columns kept -- removed and kept items every four entries of both lists."""
    _y, x = np.mgrid[0:H, 0:W]
    code = np.where(x % 4 == 3, 2000, 30000) + rng.integers(0, 8, (H, W))
    return code_frame(code)


def poses(n):
    out = [None]
    for k in range(1, n):
        a = 0.07 * k
        T = np.eye(4)
        T[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        T[:3, 3] = [0.05 * k, -0.02 * k, 0.11 * k]
        out.append(T)
    return out


def params_of(_lib, K, depth_scales, Ts):
    arr = (_lib.MdvtFrameParams * len(Ts))()
    for k, T in enumerate(Ts):
        for i, v in enumerate(np.asarray(K, np.float64).reshape(9)):
            arr[k].K[i] = v                                          # (Krender stays 0: the export does not read it)
        arr[k].depth_scale = float(depth_scales[k])
        if T is not None:
            arr[k].has_T = 1
            for i, v in enumerate(np.asarray(T, np.float64).reshape(16)):
                arr[k].T[i] = v
    return arr


def make_context(_lib, W, H, workspace_mib=0):
    ctx = _lib.Context(0, W, H)
    if workspace_mib:
        cfg = _lib.MdvtConfig()
        cfg.mode, cfg.max_depth, cfg.ipd_m, cfg.workspace_mib = 1, 100.0, 0.065, int(workspace_mib)
        ctx.call("mdvt_set_config", C.byref(cfg))
    return ctx


def capacity(name, W, H):
    return 2 * (W - 1) * (H - 1) if name == "triangles" else W * H


def export(_lib, ctx, depth, K, *, decode, remove_edges, max_depth=100.0, depth_scales=None, Ts=None, color=None, want=OUTPUTS, stream=None,
           gap=0):
    """One call on the frames depth [N, H, W, 3] (a torch CUDA tensor is taken as it is, strides and all).  Every wanted output is a
    buffer full of POISON, its frames a full list + `gap` entries apart.  -> dict(name -> host array [N, capacity + gap, ...]), counts."""
    import torch
    d = depth if isinstance(depth, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(depth)).cuda()
    N, H, W = int(d.shape[0]), int(d.shape[1]), int(d.shape[2])
    c = None
    if color is not None:
        c = color if isinstance(color, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(color)).cuda()
    opts = _lib.MdvtGeometryOpts(decode=int(decode), remove_edges=int(remove_edges), max_depth=float(max_depth))
    io = _lib.MdvtGeometryIO()
    io.depth_rgb, io.depth_pitch, io.depth_stride = d.data_ptr(), d.stride(1), d.stride(0)
    if c is not None:
        io.color_rgb, io.color_pitch, io.color_stride = c.data_ptr(), c.stride(1), c.stride(0)
    bufs = {}
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        counts = torch.full((N, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        for name in want:
            stride = (capacity(name, W, H) + gap) * ITEM[name]
            stride += -stride % 8
            bufs[name] = torch.full((N, stride), POISON, dtype=torch.uint8, device="cuda")
            setattr(io, name, bufs[name].data_ptr())
            setattr(io, {"used_index": "used_stride"}.get(name, name + "_stride"), stride)
    io.counts = counts.data_ptr()
    arr = params_of(_lib, K, depth_scales if depth_scales is not None else [1.0] * N, Ts if Ts is not None else [None] * N)
    ctx.call("mdvt_export_geometry_batch", N, arr, C.byref(opts), C.byref(io), _lib.stream_arg(d.device, stream))
    if stream is not None:
        stream.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}, counts.cpu().numpy().astype(np.int64)


_REF = {}


def reference(key, depth, K, **kw):
    """gr.export per frame, computed once per `key` and left unchanged."""
    if key not in _REF:
        Ts, scales, color = kw.pop("Ts", None), kw.pop("depth_scales", None), kw.pop("color", None)
        _REF[key] = [gr.export(depth[f], K, T=None if Ts is None else Ts[f], depth_scale=1.0 if scales is None else scales[f],
                               color_rgb=None if color is None else color[f], **kw) for f in range(len(depth))]
    return _REF[key]


def check(out, counts, refs, W, H, what=""):
    """Every output and counts bit for bit, and POISON in every byte beyond a count."""
    for f, ref in enumerate(refs):
        U, M = ref.counts
        assert (int(counts[f, 0]), int(counts[f, 1])) == (U, M), f"{what} frame {f}: counts {counts[f]} for U, M = {U}, {M}"
        for name, raw in out.items():
            n = {"vertices": W * H, "triangles": M}.get(name, U)
            want = np.ascontiguousarray(getattr(ref, name), DTYPE[name])
            got, rest = raw[f, :n * ITEM[name]], raw[f, n * ITEM[name]:]
            if got.tobytes() != want.tobytes():
                g = got.view(DTYPE[name]).reshape(want.shape)
                bits = {8: np.uint64, 4: np.uint32, 1: np.uint8}[want.dtype.itemsize]
                bad = np.argwhere(g.view(bits) != want.view(bits))
                raise AssertionError(f"{what} frame {f}: {name} differs at {len(bad)} value(s) of {want.size}, first at {bad[0]}: "
                                     f"{g[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}")
            assert np.all(rest == POISON), f"{what} frame {f}: {name} was written beyond its {n} entries ({int((rest != POISON).sum())} bytes)"
