"""The tensor contract of the Python layer: one record per public function or method that hands a tensor's address to libmdvt_hip.so,
a recorder that stores the library calls a wrapper would make without making them, and an extent checker that holds the
(pointer, pitch, stride, count, bytes per row, rows) groups of a recorded call to the bytes the tensors own.

tests/footprint.py and the far-offset tests hold the library, through the raw C ABI, to the pitches and strides it is given; what is
held here is the step before: that a caller's tensor becomes the (pointer, pitch, stride, n) it really has, and that a tensor the
docstring does not promise to take is refused before the library sees an address.

    RECORDS                         the table (tests/test_binding_contract_cpu.py holds it to the package's sources)
    Recorder                        with Recorder() as rec: ...; rec.calls -- nothing is launched inside
    owned_bytes / Touch / check_groups   the extent checker (NumPy address sets: the shapes here are a few kilobytes)
    refusal_problems / geometry_problems / result_problems   the three passes of tests/test_gpu_binding_contract.py, per record
"""
import ast
import ctypes as C
import importlib
import os
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

PKG = "metric_depth_video_toolbox_amd"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the modules whose wrappers the table covers (every module of the package that hands a tensor's address to the library)
MODULES = ("stereo_rerender", "depth_frames_helper", "infill_common", "basic_nomal_infill", "stereo_dissoclusion_net_infill",
           "stereo_crafter_infill", "m2svid_infill", "infill_clip", "find_convergence_depth", "video_metric_convert", "view_depthfile",
           "ffv1_device", "model_hop", "step_device", "geometry_device", "megasam_device", "inspatio_device")

SIZES = ((33, 5), (36, 6), (6, 6))          # W x H: odd and across a 32-pixel mask word; a multiple of 4 (vector paths); square
N_FRAMES = 3
MODEL_WH = (8, 6)                           # the model / image size of the adapter and m2svid wrappers: the smallest that differs from W x H
MASK_WH = (4, 3)
ORG_WH = (9, 7)


def mod(name):
    return importlib.import_module(f"{PKG}.{name}")


# ------------------------------------------------------------------------------------------------------------------------------------
# the recorder
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Call:
    name: str
    args: list


def plain(v):
    """A ctypes argument as the library would read it: pointers and scalars as ints, a byref() structure as a dict of its fields."""
    if hasattr(v, "_obj"):                                   # C.byref(x)
        v = v._obj
    if isinstance(v, C.Structure):
        return {f[0]: plain(getattr(v, f[0])) for f in v._fields_}
    if isinstance(v, C.c_void_p):
        return v.value or 0
    if isinstance(v, C._SimpleCData):
        return v.value
    return v


class Recorder:
    """Replaces _lib.Context.call and _lib.SharedContext.call: the calls made inside the block are stored (their arguments as
    plain() gives them) and nothing reaches the library.  prepared(job) stores the one call a PreparedRender's launch() would make,
    read from its MdvtIO, without launching it."""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        self._lib = mod("_lib")
        self._saved = (self._lib.Context.call, self._lib.SharedContext.call)
        rec = self

        def call(ctx, name, *args):
            rec.calls.append(Call(name, [plain(a) for a in args]))
        self._lib.Context.call = call
        self._lib.SharedContext.call = call
        return self

    def __exit__(self, *exc):
        self._lib.Context.call, self._lib.SharedContext.call = self._saved
        return False

    def prepared(self, job):
        self.calls.append(Call("mdvt_render_stereo_batch", [int(job._n), job._arr, plain(job._io), None]))
        return job.results


# ------------------------------------------------------------------------------------------------------------------------------------
# the extent checker
# ------------------------------------------------------------------------------------------------------------------------------------
def owned_bytes(t):
    """The addresses of the bytes a torch tensor owns, sorted, each once: from data_ptr(), shape, stride() and element_size()."""
    e = t.element_size()
    addr = np.array([t.data_ptr()], np.int64)
    for size, stride in zip(t.shape, t.stride()):
        addr = (addr[:, None] + np.arange(int(size), dtype=np.int64)[None, :] * (int(stride) * e)).reshape(-1)
    addr = (addr[:, None] + np.arange(e, dtype=np.int64)[None, :]).reshape(-1)
    return np.unique(addr)


@dataclass
class Touch:
    """What the library touches for one pointer group: `n` frames `stride` bytes apart, `planes` planes `plane` bytes apart in each
    (a planar tensor's three; one for every other), `rows` rows `pitch` bytes apart in each plane, `row_bytes` bytes in each row from
    `ptr` on."""
    ptr: int
    pitch: int
    stride: int
    n: int
    row_bytes: int
    rows: int
    planes: int = 1
    plane: int = 0

    def addresses(self):
        """Every touched address, one entry per (frame, plane, row, byte): an address two rows share is there twice."""
        f = np.arange(self.n, dtype=np.int64)[:, None, None, None] * int(self.stride if self.n > 1 else 0)
        p = np.arange(self.planes, dtype=np.int64)[None, :, None, None] * int(self.plane if self.planes > 1 else 0)
        r = np.arange(self.rows, dtype=np.int64)[None, None, :, None] * int(self.pitch if self.rows > 1 else 0)
        b = np.arange(self.row_bytes, dtype=np.int64)[None, None, None, :]
        return (int(self.ptr) + f + p + r + b).reshape(-1)

    def where(self, address):
        f, p, r, b = np.unravel_index(int(np.argmax(self.addresses() == address)), (self.n, self.planes, self.rows, self.row_bytes))
        return f"(frame {f}, {f'plane {p}, ' if self.planes > 1 else ''}row {r}, byte {b})"


def check_groups(what, tensor, touches, output, partial=False):
    """The problems of one tensor's pointer groups (all of one call's groups that name the tensor), as a list of texts -- empty
    when the library touches the tensor's own bytes and nothing else:
      a touched byte the tensor does not own (any tensor);
      an owned byte that is not touched (an output: a pixel that would be left unwritten; an input, unless `partial`: the
      library would compute from part of the tensor, which a wrong pitch or count looks like from this side);
      for an output, a byte touched twice (rows or frames that fold onto one another)."""
    own = owned_bytes(tensor)
    problems = []
    got = []
    for k, t in enumerate(touches):
        a = t.addresses()
        got.append(a)
        stray = a[~np.isin(a, own)]
        if stray.size:
            lo = int(stray.min())
            problems.append(f"{what}, group {k}: {stray.size} touched byte(s) the tensor does not own, the lowest at {t.where(lo)} = "
                            f"{lo - int(own[0]):+d} bytes from the tensor's first byte (the tensor owns {own.size} bytes over "
                            f"{int(own[-1]) - int(own[0]) + 1}; ptr {t.ptr - int(own[0]):+d}, pitch {t.pitch}, stride {t.stride}, n {t.n}, "
                            f"{f'{t.planes} planes {t.plane} apart, ' if t.planes > 1 else ''}{t.rows} rows of {t.row_bytes} bytes)")
    if not touches:
        return [f"{what}: no pointer group was recorded"]
    allgot = np.concatenate(got)
    uniq, counts = np.unique(allgot, return_counts=True)
    if not partial:
        missed = own[~np.isin(own, uniq)]
        if missed.size:
            problems.append(f"{what}: {missed.size} of the tensor's {own.size} bytes would not be {'written' if output else 'read'}, the first "
                            f"{int(missed[0]) - int(own[0])} bytes into it")
    if output and (counts > 1).any():
        problems.append(f"{what}: {int((counts > 1).sum())} byte(s) would be written more than once (rows or frames fold onto one another)")
    return problems


# ------------------------------------------------------------------------------------------------------------------------------------
# the records
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Arg:
    """One tensor argument.  kind "rgb": uint8-like [N,]h,w,3; "plane": [N,]h,w; "planar": [N,]3,h,w (a plane level between frame
    and row); "vec": `shape`, contiguous, no pixels.
    layout: what the docstring promises to take -- "strided" (pixels packed, rows and frames at any pitch), "contiguous" (no pitch
    of the tensor is passed on), "copied" (any layout: the wrapper works on a contiguous copy)."""
    name: str
    kind: str = "rgb"
    dtype: str = "uint8"
    role: str = "in"                          # "in" | "out"
    layout: str = "strided"
    batched: bool = True                      # has the leading frame dimension
    wide: int = 1                             # pixels per row = wide * W (2: two eyes side by side)
    hw: Optional[Callable] = None             # env -> (h, w) where the size is the argument's own (model frames)
    shape: Optional[Callable] = None          # env -> shape, for "vec"
    leads: bool = False                       # the call's size and frame count are this argument's: no other is wrong for it ...
    free_hw: bool = False                     # its height and width are its own (model frames); its frame count is the call's
    fixed: bool = False                       # ... unless the renderer fixes W x H
    also: tuple = ()                          # further dtypes the docstring allows ("bool")
    optional: bool = False                    # None is allowed (out=None: the wrapper allocates and returns it)
    expand: bool = True                       # an input batch made by expand() (frame stride 0): among the promised strides, or
                                              # (False) refused: the entry point takes no stride below a frame
    fewer_ok: bool = False                    # fewer frames than the call's N are allowed (a mask video that ends early)

    def dims(self, env, n=None):
        if self.kind == "vec":
            return tuple(self.shape(env))
        h, w = self.hw(env) if self.hw else (env.H, self.wide * env.W)
        lead = ((env.N if n is None else n),) if self.batched else ()
        return lead + ((3,) if self.kind == "planar" else ()) + (h, w) + ((3,) if self.kind == "rgb" else ())

    @property
    def packed(self):
        return {"rgb": 2, "plane": 1, "planar": 1, "vec": 0}[self.kind]


@dataclass(frozen=True)
class G:
    """One pointer group of a C call: where in the recorded arguments (positions after the entry point's name; a string names a field
    of the call's MdvtIO / MdvtViewIO; ("=", v) is a literal) pointer, pitch, stride and count stand, and the bytes per row and rows
    as functions of the environment; `plane`, `planes`: where a planar tensor's plane distance stands, and how many planes it has.
    `arg` names the record's argument -- or, with out=None or for returned buffers, the result --
    the group must stay inside; `offset`: bytes from the recorded pointer to the first touched one (the eye's half of a row)."""
    arg: str
    entry: str
    ptr: object
    pitch: object = None
    stride: object = None
    n: object = ("=", 1)
    row_bytes: Callable = None
    rows: Callable = lambda e: e.H
    offset: Callable = lambda e: 0
    partial: bool = False
    plane: object = None
    planes: int = 1


@dataclass
class Record:
    name: str
    sites: tuple                              # "<module>.<qualified function>" of the package's sources this record covers
    args: tuple
    call: Callable                            # (env, a: dict name -> tensor or None) -> dict name -> result
    groups: tuple
    renderer: Optional[dict] = None           # StereoRerenderer keywords where the function is a method / takes a renderer
    inplace: Optional[tuple] = None           # (input, output) the docstring allows to be one tensor
    sizes: tuple = SIZES
    setup: Optional[Callable] = None          # env -> None: what the call needs beside tensors (packets, parameter records)
    entries: tuple = ()
    min_frames: int = 1                       # the fewest frames the call takes (2: a pair of frames): the mid_frame layout's batch
                                              # of one frame is not built for such a record

    def arg(self, name):
        return next(a for a in self.args if a.name == name)


class Env:
    def __init__(self, W, H, N=N_FRAMES, device="cuda", renderer=None):
        self.W, self.H, self.N, self.device, self.r = W, H, N, device, renderer      # (device: a torch.device where a GPU is used)
        self.recorder = None
        self.MW, self.MH = MODEL_WH
        self.KW, self.KH = MASK_WH
        self.OW, self.OH = ORG_WH
        self.eye = 1
        self.extra = {}


def _rgb(name, **kw):
    return Arg(name, "rgb", **kw)


def _plane(name, dtype="uint8", **kw):
    return Arg(name, "plane", dtype, **kw)


def _out(name="out", kind="rgb", dtype="uint8", **kw):
    kw.setdefault("optional", True)
    return Arg(name, kind, dtype, role="out", **kw)


R3 = lambda e: 3 * e.W                       # noqa: E731   bytes per row of packed RGB, one eye
R1 = lambda e: e.W                           # noqa: E731
R4 = lambda e: 4 * e.W                       # noqa: E731
R6 = lambda e: 6 * e.W                       # noqa: E731


def _img_groups(entry, triples, n):
    """(arg, first position) per [pointer, pitch, stride] triple of batched packed-RGB images."""
    return tuple(G(a, entry, p, p + 1, p + 2, n, R3) for a, p in triples)


def _params(e, n=None):
    p = e.r.frame_params(xfov=45.0)
    return p if n is None else [p] * n


def _prepare(e, a):
    job = e.r.prepare(a["depth_rgb"], a["color_rgb"], _params(e, e.N), out_sbs=a["out_sbs"], out_mask=a["out_mask"], want_depth=True,
                      out_depth=a["out_depth"])
    res = e.recorder.prepared(job) if e.recorder is not None else job.launch()
    return {"out_sbs": res["sbs"], "out_mask": res["mask"], "out_depth": res["depth"]}


def _io_groups(entry, n=0):
    def g(arg, ptr, pitch, stride, rb, off=0):
        return G(arg, entry, ptr, pitch, stride, n, rb)
    return g


def _stereo_io():
    g = _io_groups("mdvt_render_stereo_batch")
    return (g("depth_rgb", "depth_rgb", "depth_pitch", "depth_stride", R3), g("color_rgb", "color_rgb", "color_pitch", "color_stride", R3),
            g("out_sbs", "left_rgb", "rgb_pitch", "rgb_stride", R3), g("out_sbs", "right_rgb", "rgb_pitch", "rgb_stride", R3),
            g("out_mask", "left_mask", "mask_pitch", "mask_stride", R1), g("out_mask", "right_mask", "mask_pitch", "mask_stride", R1),
            g("out_depth", "left_depth", "zout_pitch", "zout_stride", R4), g("out_depth", "right_depth", "zout_pitch", "zout_stride", R4))


def _view_io():
    g = _io_groups("mdvt_render_view_batch")
    return (g("depth_rgb", "depth_rgb", "depth_pitch", "depth_stride", R3), g("color_rgb", "color_rgb", "color_pitch", "color_stride", R3),
            g("rgb", "rgb", "rgb_pitch", "rgb_stride", R3), g("mask", "mask", "mask_pitch", "mask_stride", R1),
            g("depth", "depth", "zout_pitch", "zout_stride", R4),
            G("hole_counts", "mdvt_render_view_batch", "hole_counts", row_bytes=lambda e: 4 * e.N, rows=lambda e: 1))


def _finish_sbs(order):
    entry = "mdvt_finish_infill_mask_heap_stereo" if order == "heap" else "mdvt_finish_infill_mask_stereo"
    return Record(
        f"StereoRerenderer.finish_infill_mask_sbs[{order}]", ("stereo_rerender.StereoRerenderer.finish_infill_mask_sbs",),
        (_rgb("seed_sbs", wide=2, leads=True, fixed=True), _out(wide=2)),
        lambda e, a: {"out": e.r.finish_infill_mask_sbs(a["seed_sbs"], out=a["out"], order=order)},
        (G("seed_sbs", entry, 0, 2, 3, 8, R3), G("seed_sbs", entry, 1, 2, 3, 8, R3), G("out", entry, 4, 6, 7, 8, R3), G("out", entry, 5, 6, 7, 8, R3)),
        renderer=dict(infill_mask=True), entries=(entry,))


def _finish(order):
    entry = "mdvt_finish_infill_mask_heap" if order == "heap" else "mdvt_finish_infill_mask"
    return Record(
        f"StereoRerenderer.finish_infill_mask[{order}]", ("stereo_rerender.StereoRerenderer.finish_infill_mask",),
        (_rgb("seed", leads=True, fixed=True), _out()),
        lambda e, a: {"out": e.r.finish_infill_mask(a["seed"], out=a["out"], order=order)},
        _img_groups(entry, (("seed", 0), ("out", 3)), 6), renderer=dict(infill_mask=True), entries=(entry,))


def _packets(e):
    """Host-encoded FFV1 packets of N frames of the environment's size (the decode records' input) and their configuration record."""
    vio = mod("video_io")
    rng = np.random.default_rng(77)
    frames = rng.integers(0, 256, (e.N, e.H, e.W, 3), dtype=np.uint8)
    pk = [vio.encode_frame(f, slices=(1, 1)) for f in frames]
    e.extra["packets"], e.extra["config"] = [p[0] for p in pk], pk[0][1]


def _decode(stream):
    entry = "mdvt_decode_video_stream" if stream else "mdvt_decode_video_frames"
    o = 10 if stream else 9

    def call(e, a):
        fd = mod("ffv1_device")
        ctx = mod("_lib").shared_context(e.device)
        fn = fd.enqueue_decode_stream if stream else fd.enqueue_decode
        p = fn(ctx, e.extra["packets"], e.extra["config"], e.W, e.H, out=a["out"])
        if e.recorder is None:
            p.collect()
            return {"out": p.out, "flags": p.flags}
        return {"out": p.out}
    return Record(f"ffv1_device.enqueue_decode{'_stream' if stream else ''}", ("ffv1_device._enqueue_decode",), (_out(),), call,
                  (G("out", entry, o, o + 1, o + 2, 8, R3),), setup=_packets, entries=(entry,))


def _generate(image, mask, depth):
    return (image // 2 + 3).contiguous()


def _sdiss(e, a):
    return {"out": mod("stereo_dissoclusion_net_infill").sdiss_infill(a["img"], a["infill_mask"], a["depth_rgb"], _generate, out=a["out"])}


_MODEL = lambda e: (e.MH, e.MW)              # noqa: E731
_ORG = lambda e: (e.OH, e.OW)                # noqa: E731
_EYE = lambda e: e.eye * 3 * e.W             # noqa: E731


def _scr_prepare(e, a):
    image, mask, counts = mod("stereo_crafter_infill").prepare_eye(a["sbs_color"], a["sbs_mask"], e.eye, model_size=(e.MW, e.MH))
    return {"image": image, "mask": mask, "counts": counts}


def _m2s_prepare(e, a):
    image, org_image, mask, counts = mod("m2svid_infill").prepare_eye(a["sbs_color"], a["sbs_mask"], a["org"], e.eye, image_size=(e.MW, e.MH),
                                                                      mask_size=(e.KW, e.KH))
    return {"image": image, "org_image": org_image, "mask": mask, "counts": counts}


def _composite(e, a):
    mod("infill_clip").composite_eye(a["model_frames"], a["sbs_color"], a["sbs_mask"], e.eye, a["pasted"], a["blended"])
    return {"pasted": a["pasted"], "blended": a["blended"]}


def _convergence(e, a):
    means, n_sel = mod("find_convergence_depth").convergence_depths(a["depth_frames"], a["mask_frames"], counts=True)
    return {"means": means, "n_sel": n_sel}


def _codes(e, a):
    codes, depth = mod("video_metric_convert").metric_depth_codes(a["relative"], a["fit"], 100.0, want_depth=True, out=a["out"])
    return {"out": codes, "depth": depth}


def _render_view(e, a):
    views = np.stack([np.eye(4)] * e.N)
    return dict(mod("view_depthfile").render_view(a["depth_rgb"], a["color_rgb"], views, _params(e, e.N), e.r, want_depth=True, want_hole_counts=True))


def _enqueue(e, a):
    p = mod("ffv1_device").enqueue(mod("_lib").shared_context(e.device), a["frames"], slices=(1, 1))
    if e.recorder is None:
        return {"packets": p.collect(), "host_frames": p.host_frames}
    return {"packets": p.packets, "offsets": p.offsets, "sizes": p.sizes}


def _edge_filter(e, a):
    tri, unused = e.r.edge_filter(a["depth_rgb"], _params(e))
    return {"tri": tri, "unused": unused}


ONE = lambda e: 1                            # noqa: E731
_M3 = lambda e: 3 * e.MW                     # noqa: E731
_MROWS = lambda e: e.MH                      # noqa: E731


# ---- step_device and geometry_device: the wrappers take the clip's context first; a size the clip does not fix is the model's
# (8 x 6), the mask's (4 x 3: MVSAnywhere's cost volume and its mask) or the original's (9 x 7: the video's), never W x H ----
_M4 = lambda e: 4 * e.MW                     # noqa: E731
_O3 = lambda e: 3 * e.OW                     # noqa: E731
_O4 = lambda e: 4 * e.OW                     # noqa: E731
_OROWS = lambda e: e.OH                      # noqa: E731
_MASK = lambda e: (e.KH, e.KW)               # noqa: E731
_NVEC = lambda e: 4 * e.N                    # noqa: E731


def _ctx(e, sized=False):
    """The context the step wrappers take first (the geometry wrappers': of the frames' size, which the entry points read from it)."""
    return mod("_lib").shared_context(e.device, e.W, e.H) if sized else mod("_lib").shared_context(e.device)


def _frames_in(name="frames"):
    return _rgb(name, leads=True, expand=False)


def _planes_in(name="planes", **kw):
    return _plane(name, "float32", expand=False, **kw)


def _sink(e, a):
    codes, plane = mod("step_device").depth_video_codes(_ctx(e), a["planes"], 100.0, (e.OW, e.OH), scale=a["scale"], want_plane=True, out=a["out"])
    return {"out": codes, "plane": plane}


def _model_frames(as_float):
    entry, el = "mdvt_model_frames", 4 if as_float else 1
    return Record(f"step_device.model_frames[{'float' if as_float else 'u8'}]", ("step_device.model_frames",), (_frames_in(),),
                  lambda e, a: {"out": mod("step_device").model_frames(_ctx(e), a["frames"], (e.MW, e.MH), as_float=as_float)},
                  (G("frames", entry, 3, 4, 5, 2, R3), G("out", entry, 10, 11, 13, 2, lambda e: el * e.MW, _MROWS, plane=12, planes=3)))


def _focal(planar):
    entry = "mdvt_focal_from_points"

    def call(e, a):
        focal, counts = mod("step_device").focal_from_points(_ctx(e), a["points"], want_counts=True)
        return {"focal": focal, "counts": counts}
    points = Arg("points", "planar", "float32", leads=True, expand=False) if planar else _rgb("points", dtype="float32", leads=True, expand=False)
    group = G("points", entry, 3, 5, 7, 2, R4, plane=6, planes=3) if planar else G("points", entry, 3, 5, 7, 2, lambda e: 12 * e.W)
    return Record(f"step_device.focal_from_points[{'N3HW' if planar else 'NHW3'}]", ("step_device.focal_from_points",), (points,), call,
                  (group, G("focal", entry, 8, row_bytes=lambda e: 8 * e.N, rows=ONE), G("counts", entry, 9, row_bytes=lambda e: 8 * e.N, rows=ONE)))


def _lanczos(ch):
    entry = "mdvt_lanczos_resize_u8"

    def call(e, a):
        out, form = mod("step_device").lanczos_resize(_ctx(e), a["images"], (e.MW, e.MH))
        return {"out": out} if e.recorder is not None else {"out": out, "form": form}      # (recorded only, no form comes back)
    images = _frames_in("images") if ch == 3 else _plane("images", leads=True, expand=False)
    return Record(f"step_device.lanczos_resize[{'RGB' if ch == 3 else 'L'}]", ("step_device.lanczos_resize",), (images,), call,
                  (G("images", entry, 4, 5, 6, 3, lambda e: ch * e.W), G("out", entry, 9, 10, 11, 3, lambda e: ch * e.MW, _MROWS)))


def _mask_from_prediction(ch):
    entry = "mdvt_mask_from_prediction"
    return Record(f"step_device.mask_from_prediction[{ch}]", ("step_device.mask_from_prediction",), (_planes_in("pred", leads=True),),
                  lambda e, a: {"out": mod("step_device").mask_from_prediction(_ctx(e), a["pred"], (e.OW, e.OH), channels=ch)},
                  (G("pred", entry, 3, 4, 5, 2, R4), G("out", entry, 9, 10, 11, 2, lambda e: ch * e.OW, _OROWS)))


def _nearest(e, a):
    codes, plane = mod("step_device").nearest_depth_codes(_ctx(e), a["planes"], (e.KW, e.KH), 100.0, (e.OW, e.OH), scale=a["scale"], want_plane=True,
                                                          out=a["out"])
    return {"out": codes, "plane": plane}


def _ratio_median(e, a):
    median, counts = mod("step_device").ratio_median(_ctx(e), a["cv"], a["ref"], a["mask"], want_counts=True, out=a["out"])
    return {"out": median, "counts": counts}


def _export(e, a):
    """The enqueueing half of export_batch.  Recorded: the five buffers as they are; launched: what export_batch reads of them --
    the counts, every vertex, and of the other lists the entries the counts name (the rest is never written)."""
    K = ((40.0, 0.0, e.W / 2), (0.0, 40.0, e.H / 2), (0.0, 0.0, 1.0))
    got = mod("geometry_device").enqueue_export(_ctx(e, True), a["depth"], a["color"], K, [None] * e.N, max_depth=100.0, remove_edges=True)
    res = dict(zip(("counts", "vertices", "triangles", "points", "point_rgb"), got))
    if e.recorder is None:
        import torch
        c = res["counts"].cpu().numpy()
        res["triangles"] = torch.cat([res["triangles"][k, :c[k, 1]] for k in range(e.N)])
        for name in ("points", "point_rgb"):
            res[name] = torch.cat([res[name][k, :c[k, 0]] for k in range(e.N)])
    return res


def _export_io():
    entry = "mdvt_export_geometry_batch"

    def lists(name, per_frame):
        return G(name, entry, name, None, name + "_stride", 0, per_frame, ONE)
    return (G("depth", entry, "depth_rgb", "depth_pitch", "depth_stride", 0, R3), G("color", entry, "color_rgb", "color_pitch", "color_stride", 0, R3),
            G("counts", entry, "counts", row_bytes=lambda e: 8 * e.N, rows=ONE),
            lists("vertices", lambda e: 24 * e.W * e.H), lists("triangles", lambda e: 24 * (e.W - 1) * (e.H - 1)),
            lists("points", lambda e: 24 * e.W * e.H), lists("point_rgb", lambda e: 3 * e.W * e.H))


def _grey(bits):
    entry = "mdvt_depth_grey_batch"
    return Record(f"geometry_device.grey_batch[{bits}]", ("geometry_device.grey_batch",), (_rgb("depth", layout="contiguous", leads=True, fixed=True),),
                  lambda e, a: {"out": mod("geometry_device").grey_batch(_ctx(e, True), a["depth"], max_depth=100.0, bits=bits)},
                  (G("depth", entry, 1, 2, 3, 0, R3), G("out", entry, 6, 7, 8, 0, lambda e: (2 if bits == 16 else 3) * e.W)))


# ---- the scene, tracker and InSpatio wrappers.  Several of their entry points refuse the table's sizes, so these keep the three kinds
# (odd across a 32-pixel word, a multiple of 4, square) at sizes of their own: an eye of 8 x 8 and more for the shift grid and the
# blend; for cv2's area resize to 8 x 6 a frame no smaller than that on either axis whose two ratios are not both integers ----
EYE_SIZES = ((33, 9), (36, 12), (8, 8))
AREA_SIZES = ((33, 9), (36, 10), (10, 10))
_K4 = lambda e: 4 * e.KW                     # noqa: E731
_KROWS = lambda e: e.KH                      # noqa: E731


def _frame_sums(with_prev):
    """sums has a row per pair: N - 1, and one more with a previous frame (unbatched, of the frames' size, on their device)."""
    entry = "mdvt_scene_frame_sums"
    return Record(f"step_device.frame_sums[{'prev' if with_prev else 'no prev'}]", ("step_device.frame_sums",),
                  (_frames_in(),) + ((_rgb("prev", batched=False),) if with_prev else ()),
                  lambda e, a: {"sums": mod("step_device").frame_sums(_ctx(e), a["frames"], a.get("prev"))},
                  (G("frames", entry, 3, 4, 5, 2, R3),) + ((G("prev", entry, 7, 8, row_bytes=R3),) if with_prev else ()) +
                  (G("sums", entry, 10, row_bytes=lambda e: 24 * (e.N - 1 + with_prev), rows=ONE),), min_frames=2)


def _tracker_in(fn, name, o, *extra):
    """tracker_depth and tracker_mask: frames -> float32 planes at the crop (4 x 3) of the tracker's size (8 x 6); `o`: where the
    output's pointer stands."""
    entry = "mdvt_" + fn
    return Record(f"megasam_device.{fn}", (f"megasam_device.{fn}",), (_frames_in(name),),
                  lambda e, a: {"out": getattr(mod("megasam_device"), fn)(_ctx(e), a[name], *extra, (e.MW, e.MH), (e.KW, e.KH))},
                  (G(name, entry, 3, 4, 5, 2, R3), G("out", entry, o, o + 1, o + 2, 2, _K4, _KROWS)))


def _tracker_outputs(mode):
    entry = "mdvt_tracker_outputs"
    return Record(f"megasam_device.tracker_outputs[{'grey' if mode else 'depth'}]", ("megasam_device.tracker_outputs",),
                  (_planes_in(leads=True), _out(hw=_ORG)),
                  lambda e, a: {"out": mod("megasam_device").tracker_outputs(_ctx(e), a["planes"], mode, 4.0 if mode else 100.0, (e.OW, e.OH), out=a["out"])},
                  (G("planes", entry, 4, 5, 6, 3, R4), G("out", entry, 10, 11, 12, 3, _O3, _OROWS)))


def _shift_grid(path):
    entry = "mdvt_masked_shift_grid"

    def call(e, a):
        shift, status, err = mod("inspatio_device").masked_shift_grid(_ctx(e), a["render"], a["infilled"], a["valid"], path=path)
        return {"shift": shift, "status": status, "round_error": err}
    return Record(f"inspatio_device.masked_shift_grid[{'direct' if path == 1 else 'transform'}]", ("inspatio_device.masked_shift_grid",),
                  (_frames_in("render"), _rgb("infilled", expand=False), _plane("valid", expand=False)), call,
                  (G("render", entry, 3, 4, 5, 2, R3), G("infilled", entry, 6, 7, 8, 2, R3), G("valid", entry, 9, 10, 11, 2, R1),
                   G("shift", entry, 13, row_bytes=lambda e: 256 * e.N, rows=ONE), G("status", entry, 14, row_bytes=lambda e: 16 * e.N, rows=ONE),
                   G("round_error", entry, 15, row_bytes=lambda e: 8, rows=ONE)), sizes=EYE_SIZES)


def _inspatio_prepare(eye):
    entry = "mdvt_inspatio_prepare_eye"
    half = dict(offset=lambda e: eye * 3 * e.W, partial=True)

    def call(e, a):
        got = mod("inspatio_device").prepare_eye(_ctx(e), a["sbs_color"], a["sbs_mask"], eye, (e.MW, e.MH))
        return dict(zip(("valid", "render", "model_valid", "model_render", "hole_counts"), got))
    return Record(f"inspatio_device.prepare_eye[{eye}]", ("inspatio_device.prepare_eye",),
                  (_rgb("sbs_color", wide=2, leads=True, expand=False), _rgb("sbs_mask", wide=2, expand=False)), call,
                  (G("sbs_color", entry, 4, 5, 6, 2, R3, **half), G("sbs_mask", entry, 7, 8, 9, 2, R3, **half),
                   G("valid", entry, 12, 13, 14, 2, R1), G("render", entry, 15, 16, 17, 2, R3),
                   G("model_valid", entry, 18, 19, 20, 2, lambda e: e.MW, _MROWS), G("model_render", entry, 21, 22, 23, 2, _M3, _MROWS),
                   G("hole_counts", entry, 24, row_bytes=_NVEC, rows=ONE)))


def _inspatio_composite(eye, blend):
    """The eye's half of `pasted` and, with `blend`, of `blended` is written."""
    entry = "mdvt_inspatio_composite_eye"
    half = dict(offset=lambda e: eye * 3 * e.W, partial=True)
    sbs = ("sbs_color", "sbs_mask", "pasted") + (("blended",) if blend else ())

    def call(e, a):
        pasted, blended = mod("inspatio_device").composite_eye(_ctx(e), a["aligned"], a["sbs_color"], a["sbs_mask"], eye, a["pasted"], a.get("blended"))
        return {"pasted": pasted, "blended": blended} if blend else {"pasted": pasted}
    return Record(f"inspatio_device.composite_eye[{eye}, {'blended' if blend else 'pasted only'}]", ("inspatio_device.composite_eye",),
                  (_frames_in("aligned"),) + tuple(_rgb(n, wide=2, expand=False) for n in sbs[:2]) + tuple(_out(n, wide=2, optional=False) for n in sbs[2:]),
                  call, (G("aligned", entry, 4, 5, 6, 2, R3),) + tuple(G(n, entry, 7 + 3 * k, 8 + 3 * k, 9 + 3 * k, 2, R3, **half) for k, n in enumerate(sbs)),
                  sizes=EYE_SIZES)


RECORDS = (
    # ---- stereo_rerender: module functions ------------------------------------------------------------------------------------------
    Record("stereo_rerender.infill_using_normals", ("stereo_rerender.infill_using_normals",),
           (_rgb("color_img", layout="copied", batched=False, leads=True), _plane("hole_mask", layout="copied", batched=False, also=("bool",)),
            _rgb("normal_map", dtype="float32", layout="copied", batched=False), _out(layout="contiguous", batched=False)),
           lambda e, a: {"out": mod("stereo_rerender").infill_using_normals(a["color_img"], a["hole_mask"], a["normal_map"], out=a["out"])},
           (G("color_img", "mdvt_infill_using_normals", 0, 1, row_bytes=R3), G("hole_mask", "mdvt_infill_using_normals", 2, 3, row_bytes=R1),
            G("normal_map", "mdvt_infill_using_normals", 4, 5, row_bytes=lambda e: 12 * e.W), G("out", "mdvt_infill_using_normals", 6, 7, row_bytes=R3))),
    Record("stereo_rerender.infill_using_mask_normals", ("stereo_rerender.infill_using_mask_normals",),
           (_rgb("img", leads=True), _plane("hole_mask", also=("bool",)), _rgb("infill_mask"), _out()),
           lambda e, a: {"out": mod("stereo_rerender").infill_using_mask_normals(a["img"], a["hole_mask"], a["infill_mask"], out=a["out"])},
           (G("out", "mdvt_infill_using_mask_normals", 0, 1, 2, 9, R3), G("hole_mask", "mdvt_infill_using_mask_normals", 3, 4, 5, 9, R1),
            G("infill_mask", "mdvt_infill_using_mask_normals", 6, 7, 8, 9, R3)), inplace=("img", "out")),
    Record("stereo_rerender.touchly_depth", ("stereo_rerender.touchly_depth",),
           (_plane("depth", "float32", batched=False, leads=True), _out(layout="contiguous", batched=False)),
           lambda e, a: {"out": mod("stereo_rerender").touchly_depth(a["depth"], out=a["out"])},
           (G("depth", "mdvt_touchly_depth", 0, 1, row_bytes=R4), G("out", "mdvt_touchly_depth", 2, 3, row_bytes=R3))),
    Record("stereo_rerender.convert_to_equirectangular", ("stereo_rerender.convert_to_equirectangular",),
           (_rgb("image", leads=True), _out()),
           lambda e, a: {"out": mod("stereo_rerender").convert_to_equirectangular(a["image"], out=a["out"])},
           _img_groups("mdvt_equirect_remap", (("image", 0), ("out", 3)), 6)),
    Record("stereo_rerender.masked_blur", ("stereo_rerender.masked_blur",),
           (_rgb("img", batched=False, leads=True), _out(batched=False)),
           lambda e, a: {"out": mod("stereo_rerender").masked_blur(a["img"], out=a["out"])},
           (G("img", "mdvt_masked_blur", 0, 1, row_bytes=R3), G("out", "mdvt_masked_blur", 2, 3, row_bytes=R3))),
    # ---- stereo_rerender: the renderer ----------------------------------------------------------------------------------------------
    Record("StereoRerenderer.prepare", ("stereo_rerender.StereoRerenderer.prepare",),
           (_rgb("depth_rgb", layout="contiguous", leads=True, fixed=True), _rgb("color_rgb", layout="contiguous"),
            _out("out_sbs", layout="contiguous", wide=2), _out("out_mask", "plane", layout="contiguous", wide=2),
            _out("out_depth", "plane", "float32", layout="contiguous", wide=2)),
           _prepare, _stereo_io(), renderer={}, entries=("mdvt_render_stereo_batch",)),
    _finish_sbs("levels"), _finish_sbs("heap"), _finish("levels"), _finish("heap"),
    Record("StereoRerenderer.edge_filter", ("stereo_rerender.StereoRerenderer.edge_filter",),
           (_rgb("depth_rgb", layout="contiguous", batched=False, leads=True, fixed=True),), _edge_filter,
           (G("depth_rgb", "mdvt_edge_filter", 0, 1, row_bytes=R3),
            G("tri", "mdvt_edge_filter", 5, row_bytes=lambda e: 2 * (e.H - 1) * (e.W - 1), rows=ONE),
            G("unused", "mdvt_edge_filter", 6, row_bytes=lambda e: e.H * e.W, rows=ONE)), renderer=dict(remove_edges=True)),
    Record("StereoRerenderer.edge_point_pixels", ("stereo_rerender.StereoRerenderer.edge_point_pixels",),
           (_rgb("depth_rgb", layout="contiguous", batched=False, leads=True, fixed=True),),
           lambda e, a: {"px": e.r.edge_point_pixels(a["depth_rgb"], _params(e))},
           (G("depth_rgb", "mdvt_edge_point_pixels", 1, 2, row_bytes=R3),
            G("px", "mdvt_edge_point_pixels", 4, row_bytes=lambda e: 16 * e.H * e.W, rows=ONE)), renderer=dict(remove_edges=True)),
    # ---- depth_frames_helper, infill_common, basic_nomal_infill ---------------------------------------------------------------------
    Record("depth_frames_helper.decode_rgb_depth_frame", ("depth_frames_helper.decode_rgb_depth_frame",),
           (_rgb("rgb", layout="contiguous", batched=False, leads=True), _out("out", "plane", "float32", layout="contiguous", batched=False)),
           lambda e, a: {"out": mod("depth_frames_helper").decode_rgb_depth_frame(a["rgb"], 100, out=a["out"])},
           (G("rgb", "mdvt_decode_depth", 0, 1, row_bytes=R3), G("out", "mdvt_decode_depth", 2, 3, row_bytes=R4))),
    Record("depth_frames_helper.encode_depth_frame", ("depth_frames_helper.encode_depth_frame",),
           (_plane("depth", "float32", layout="contiguous", batched=False, leads=True), _out(layout="contiguous", batched=False)),
           lambda e, a: {"out": mod("depth_frames_helper").encode_depth_frame(a["depth"], 100, out=a["out"])},
           (G("depth", "mdvt_encode_depth", 0, 1, row_bytes=R4), G("out", "mdvt_encode_depth", 2, 3, row_bytes=R3))),
    Record("depth_frames_helper.swap_rb", ("depth_frames_helper.swap_rb",), (_rgb("frames", leads=True), _out()),
           lambda e, a: {"out": mod("depth_frames_helper").swap_rb(a["frames"], out=a["out"])},
           _img_groups("mdvt_swap_rb", (("frames", 0), ("out", 3)), 6), inplace=("frames", "out")),
    Record("infill_common.mark_lower_side", ("infill_common.mark_lower_side",),
           (_rgb("normals_img", layout="copied", batched=False, leads=True), _out(layout="contiguous", batched=False)),
           lambda e, a: {"out": mod("infill_common").mark_lower_side(a["normals_img"], out=a["out"])},
           (G("normals_img", "mdvt_mark_lower_side", 0, 1, row_bytes=R3), G("out", "mdvt_mark_lower_side", 2, 3, row_bytes=R3))),
    Record("basic_nomal_infill.normal_infill", ("basic_nomal_infill.normal_infill",), (_rgb("img", leads=True), _rgb("infill_mask"), _out()),
           lambda e, a: {"out": mod("basic_nomal_infill").normal_infill(a["img"], a["infill_mask"], out=a["out"])},
           _img_groups("mdvt_normal_infill", (("img", 0), ("infill_mask", 3), ("out", 6)), 9)),
    # ---- the model infill steps -----------------------------------------------------------------------------------------------------
    Record("stereo_dissoclusion_net_infill.decode_depth_percent", ("stereo_dissoclusion_net_infill.decode_depth_percent",),
           (_rgb("depth_rgb", leads=True), _out("out", "plane", "float32", layout="contiguous")),
           lambda e, a: {"out": mod("stereo_dissoclusion_net_infill").decode_depth_percent(a["depth_rgb"], out=a["out"])},
           (G("depth_rgb", "mdvt_decode_depth", 0, 1, row_bytes=R3), G("out", "mdvt_decode_depth", 2, 3, row_bytes=R4))),
    Record("stereo_dissoclusion_net_infill.model_infill_finish", ("stereo_dissoclusion_net_infill.model_infill_finish",),
           (_rgb("img", leads=True, expand=False), _rgb("model", expand=False), _rgb("infill_mask", expand=False), _out()),
           lambda e, a: {"out": mod("stereo_dissoclusion_net_infill").model_infill_finish(a["img"], a["model"], a["infill_mask"], out=a["out"])},
           _img_groups("mdvt_model_infill_finish", (("img", 3), ("model", 6), ("infill_mask", 9), ("out", 12)), 2)),
    # (sdiss_infill hands the model contiguous copies and the library the caller's own views: its geometry is the views')
    Record("stereo_dissoclusion_net_infill.sdiss_infill", (), (_rgb("img", leads=True, expand=False), _rgb("infill_mask", expand=False), _rgb("depth_rgb"), _out()), _sdiss,
           (G("depth_rgb", "mdvt_decode_depth", 0, 1, row_bytes=R3),) +
           _img_groups("mdvt_model_infill_finish", (("img", 3), ("infill_mask", 9), ("out", 12)), 2)),
    Record("stereo_crafter_infill.prepare_eye", ("stereo_crafter_infill.prepare_eye",), (_rgb("sbs_color", wide=2, leads=True, expand=False), _rgb("sbs_mask", wide=2, expand=False)),
           _scr_prepare,
           (G("sbs_color", "mdvt_adapter_prepare_eye", 4, 5, 6, 2, R3, offset=_EYE, partial=True),
            G("sbs_mask", "mdvt_adapter_prepare_eye", 7, 8, 9, 2, R3, offset=_EYE, partial=True),
            G("image", "mdvt_adapter_prepare_eye", 12, 13, 14, 2, _M3, _MROWS),
            G("mask", "mdvt_adapter_prepare_eye", 15, 16, 17, 2, lambda e: e.MW, _MROWS),
            G("counts", "mdvt_adapter_prepare_eye", 18, row_bytes=lambda e: 4 * e.N, rows=ONE))),
    Record("stereo_crafter_infill.lhm_moments", ("stereo_crafter_infill.lhm_moments",),
           (_rgb("frames", leads=True, expand=False), _plane("mask", expand=False), _out("out", "vec", "int64", layout="contiguous", shape=lambda e: (e.N, 10))),
           lambda e, a: {"out": mod("stereo_crafter_infill").lhm_moments(a["frames"], a["mask"], out=a["out"])},
           (G("frames", "mdvt_lhm_moments", 3, 4, 5, 2, R3), G("mask", "mdvt_lhm_moments", 6, 7, 8, 2, R1),
            G("out", "mdvt_lhm_moments", 9, row_bytes=lambda e: 80 * e.N, rows=ONE))),
    Record("stereo_crafter_infill.lhm_apply", ("stereo_crafter_infill.lhm_apply",),
           (_rgb("frames", leads=True, expand=False), Arg("params", "vec", "float64", layout="contiguous", shape=lambda e: (e.N, 15)), _out()),
           lambda e, a: {"out": mod("stereo_crafter_infill").lhm_apply(a["frames"], a["params"], out=a["out"])},
           (G("frames", "mdvt_lhm_apply", 3, 4, 5, 2, R3), G("params", "mdvt_lhm_apply", 6, row_bytes=lambda e: 120 * e.N, rows=ONE),
            G("out", "mdvt_lhm_apply", 7, 8, 9, 2, R3))),
    Record("m2svid_infill.prepare_eye", ("m2svid_infill.prepare_eye",),
           (_rgb("sbs_color", wide=2, leads=True, expand=False), _rgb("sbs_mask", wide=2, expand=False),
            _rgb("org", hw=_ORG, free_hw=True, expand=False)), _m2s_prepare,
           (G("sbs_color", "mdvt_m2svid_prepare_eye", 4, 5, 6, 2, R3, offset=_EYE, partial=True),
            G("sbs_mask", "mdvt_m2svid_prepare_eye", 7, 8, 9, 2, R3, offset=_EYE, partial=True),
            G("org", "mdvt_m2svid_prepare_eye", 10, 13, 14, 2, lambda e: 3 * e.OW, lambda e: e.OH),
            G("image", "mdvt_m2svid_prepare_eye", 19, 20, 21, 2, _M3, _MROWS), G("org_image", "mdvt_m2svid_prepare_eye", 22, 23, 24, 2, _M3, _MROWS),
            G("mask", "mdvt_m2svid_prepare_eye", 25, 26, 27, 2, lambda e: e.KW, lambda e: e.KH),
            G("counts", "mdvt_m2svid_prepare_eye", 28, row_bytes=lambda e: 4 * e.N, rows=ONE))),
    Record("infill_clip.composite_eye", ("infill_clip.composite_eye",),
           (_rgb("model_frames", hw=_MODEL, free_hw=True, expand=False), _rgb("sbs_color", wide=2, leads=True, expand=False),
            _rgb("sbs_mask", wide=2, expand=False),
            _out("pasted", wide=2, optional=False), _out("blended", wide=2, optional=False)), _composite,
           (G("model_frames", "mdvt_adapter_composite_eye", 4, 7, 8, 2, _M3, _MROWS),
            G("sbs_color", "mdvt_adapter_composite_eye", 9, 10, 11, 2, R3, offset=_EYE, partial=True),
            G("sbs_mask", "mdvt_adapter_composite_eye", 12, 13, 14, 2, R3, offset=_EYE, partial=True),
            G("pasted", "mdvt_adapter_composite_eye", 15, 16, 17, 2, R3, offset=_EYE, partial=True),
            G("blended", "mdvt_adapter_composite_eye", 18, 19, 20, 2, R3, offset=_EYE, partial=True)),
           sizes=((33, 9), (36, 8), (8, 8))),          # (the library's blend takes eyes of 8 x 8 and more: its 15-tap Gaussian's reflection)
    # ---- find_convergence_depth, video_metric_convert, view_depthfile ---------------------------------------------------------------
    Record("find_convergence_depth.convergence_depths", ("find_convergence_depth.convergence_depths",),
           (_rgb("depth_frames", leads=True, expand=False), _rgb("mask_frames", expand=False, fewer_ok=True)), _convergence,
           (G("depth_frames", "mdvt_convergence_depths", 2, 3, 4, 10, R3), G("mask_frames", "mdvt_convergence_depths", 6, 7, 8, 11, R3),
            G("means", "mdvt_convergence_depths", 13, row_bytes=lambda e: 4 * e.N, rows=ONE),
            G("n_sel", "mdvt_convergence_depths", 14, row_bytes=lambda e: 4 * e.N, rows=ONE))),
    Record("video_metric_convert.compute_scale_and_shift_full", ("video_metric_convert.compute_scale_and_shift_full",),
           (_plane("prediction", "float32", leads=True, expand=False), _plane("target", "float32", expand=False),
            _plane("mask", also=("bool",), expand=False)),
           lambda e, a: {"fit": mod("video_metric_convert").compute_scale_and_shift_full(a["prediction"], a["target"], a["mask"]).values},
           (G("prediction", "mdvt_scale_shift_fit", 3, 4, 5, 2, R4), G("target", "mdvt_scale_shift_fit", 6, 7, 8, 2, R4),
            G("mask", "mdvt_scale_shift_fit", 10, 11, 12, 2, R1), G("fit", "mdvt_scale_shift_fit", 13, row_bytes=lambda e: 32, rows=ONE))),
    Record("video_metric_convert.metric_depth_codes", ("video_metric_convert.metric_depth_codes",),
           (_plane("relative", "float32", leads=True, expand=False), Arg("fit", "vec", "float32", layout="contiguous", shape=lambda e: (8,)), _out()), _codes,
           (G("relative", "mdvt_metric_depth_codes", 3, 4, 5, 2, R4),
            G("fit", "mdvt_metric_depth_codes", 6, row_bytes=lambda e: 8, rows=ONE, partial=True),
            G("out", "mdvt_metric_depth_codes", 11, 12, 13, 2, R3), G("depth", "mdvt_metric_depth_codes", 15, 16, 17, 2, R4))),
    Record("view_depthfile.centers", ("view_depthfile.centers",), (_rgb("depth_rgb", leads=True, fixed=True, expand=False),),
           lambda e, a: {"centers": mod("view_depthfile").centers(a["depth_rgb"], _params(e, e.N), e.r)},
           (G("depth_rgb", "mdvt_view_centers", 2, 3, 4, 0, R3), G("centers", "mdvt_view_centers", 5, row_bytes=lambda e: 24 * e.N, rows=ONE)),
           renderer=dict(pupillary_distance=0, dont_place_points_in_edges=True)),
    Record("view_depthfile.render_view", ("view_depthfile.render_view",), (_rgb("depth_rgb", leads=True, fixed=True, expand=False), _rgb("color_rgb", expand=False)),
           _render_view, _view_io(), renderer=dict(pupillary_distance=0, dont_place_points_in_edges=True), entries=("mdvt_render_view_batch",)),
    # ---- ffv1_device, model_hop -----------------------------------------------------------------------------------------------------
    # (enqueue hands the kernel the layouts it reads -- dense pixels, padded rows and frames -- and encodes any other from a contiguous copy)
    Record("ffv1_device.enqueue", ("ffv1_device.enqueue",), (_rgb("frames", layout="copied", leads=True),), _enqueue,
           (G("frames", "mdvt_encode_video_frames", 4, 5, 6, 9, R3),
            G("packets", "mdvt_encode_video_frames", 11, row_bytes=lambda e: e.extra["cap"], rows=ONE),
            G("offsets", "mdvt_encode_video_frames", 13, row_bytes=lambda e: 8 * e.N, rows=ONE),
            G("sizes", "mdvt_encode_video_frames", 14, row_bytes=lambda e: 4 * e.N, rows=ONE)),
           setup=lambda e: e.extra.update(cap=e.N * mod("ffv1_device").packet_capacity_bytes(e.W, e.H, (1, 1)))),
    _decode(False), _decode(True),
    Record("model_hop.depth_to_rgb_code", ("model_hop.depth_to_rgb_code",),
           (_plane("depth", "float32", layout="contiguous", leads=True), _out(layout="contiguous")),
           lambda e, a: {"out": mod("model_hop").depth_to_rgb_code(a["depth"], 100.0, out=a["out"])},
           (G("depth", "mdvt_encode_depth", 0, 1, row_bytes=R4, rows=lambda e: e.N * e.H), G("out", "mdvt_encode_depth", 2, 3, row_bytes=R3, rows=lambda e: e.N * e.H))),
    # ---- step_device: the model steps' wrappers (no entry point of theirs takes a stride below a frame: expand=False) ---------------
    Record("step_device.depth_video_codes", ("step_device.depth_video_codes",),
           (_planes_in(leads=True), Arg("scale", "vec", "float32", layout="contiguous", shape=lambda e: (1,)), _out(hw=_ORG)), _sink,
           (G("planes", "mdvt_depth_video_codes", 3, 4, 5, 2, R4), G("scale", "mdvt_depth_video_codes", 6, row_bytes=lambda e: 4, rows=ONE),
            G("out", "mdvt_depth_video_codes", 11, 12, 13, 2, _O3, _OROWS), G("plane", "mdvt_depth_video_codes", 15, 16, 17, 2, _O4, _OROWS))),
    _model_frames(False), _model_frames(True),
    Record("step_device.depth_prompt", ("step_device.depth_prompt",), (_frames_in("codes"),),
           lambda e, a: {"out": mod("step_device").depth_prompt(_ctx(e), a["codes"], 100.0, (e.MW, e.MH))},
           (G("codes", "mdvt_depth_prompt", 3, 4, 5, 2, R3), G("out", "mdvt_depth_prompt", 10, 11, 12, 2, _M4, _MROWS))),
    _focal(False), _focal(True), _lanczos(1), _lanczos(3),
    Record("step_device.mask_model_input", ("step_device.mask_model_input",), (_frames_in(),),
           lambda e, a: {"out": mod("step_device").mask_model_input(_ctx(e), a["frames"], (e.MW, e.MH), (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))},
           (G("frames", "mdvt_mask_model_input", 3, 4, 5, 2, R3), G("out", "mdvt_mask_model_input", 11, 12, 14, 2, _M4, _MROWS, plane=13, planes=3))),
    _mask_from_prediction(1), _mask_from_prediction(3),
    # (out: a slice of the tool's ring of planar model frames)
    Record("step_device.bilinear_model_frames", ("step_device.bilinear_model_frames",), (_frames_in(), _out("out", "planar", "float32", hw=_MODEL)),
           lambda e, a: {"out": mod("step_device").bilinear_model_frames(_ctx(e), a["frames"], (e.MW, e.MH), out=a["out"])},
           (G("frames", "mdvt_bilinear_model_frames", 3, 4, 5, 2, R3),
            G("out", "mdvt_bilinear_model_frames", 9, 10, 12, 2, _M4, _MROWS, plane=11, planes=3))),
    Record("step_device.nearest_depth_codes", ("step_device.nearest_depth_codes",),
           (_planes_in(leads=True), Arg("scale", "vec", "float32", layout="contiguous", shape=lambda e: (e.N,)), _out(hw=_ORG)), _nearest,
           (G("planes", "mdvt_nearest_depth_codes", 3, 4, 5, 2, R4), G("scale", "mdvt_nearest_depth_codes", 8, None, 9, 2, lambda e: 4, ONE),
            G("out", "mdvt_nearest_depth_codes", 13, 14, 15, 2, _O3, _OROWS), G("plane", "mdvt_nearest_depth_codes", 17, 18, 19, 2, _O4, _OROWS))),
    Record("step_device.ratio_median", ("step_device.ratio_median",),
           (_planes_in("cv", leads=True), _planes_in("ref", hw=_MODEL, free_hw=True), _plane("mask", hw=_MASK, free_hw=True, expand=False),
            _out("out", "vec", "float32", layout="contiguous", shape=lambda e: (e.N,))), _ratio_median,
           (G("cv", "mdvt_ratio_median", 3, 4, 5, 0, R4), G("ref", "mdvt_ratio_median", 8, 9, 10, 0, _M4, _MROWS),
            G("mask", "mdvt_ratio_median", 13, 14, 15, 0, lambda e: e.KW, lambda e: e.KH),
            G("out", "mdvt_ratio_median", 16, row_bytes=_NVEC, rows=ONE), G("counts", "mdvt_ratio_median", 17, row_bytes=_NVEC, rows=ONE))),
    # ---- geometry_device: the context fixes W x H, the library is told no pitch of the tensors' own ---------------------------------
    Record("geometry_device.enqueue_export", ("geometry_device.enqueue_export",),
           (_rgb("depth", layout="contiguous", leads=True, fixed=True), _rgb("color", layout="contiguous")), _export, _export_io()),
    _grey(8), _grey(16),
    # ---- step_device.frame_sums, megasam_device, inspatio_device: as step_device's (the context first, expand=False) ----------------
    _frame_sums(False), _frame_sums(True),
    # (the crop 4 x 3 is smaller than the tracker's size 8 x 6: a wrapper that dropped it would write 8 x 6)
    Record("megasam_device.area_model_frames", ("megasam_device.area_model_frames",), (_frames_in(),),
           lambda e, a: {"out": mod("megasam_device").area_model_frames(_ctx(e), a["frames"], (e.MW, e.MH), (e.KW, e.KH))},
           (G("frames", "mdvt_area_model_frames", 3, 4, 5, 2, R3),
            G("out", "mdvt_area_model_frames", 11, 12, 14, 2, lambda e: e.KW, _KROWS, plane=13, planes=3)), sizes=AREA_SIZES),
    _tracker_in("tracker_depth", "codes", 12, 100.0), _tracker_in("tracker_mask", "masks", 11),
    _tracker_outputs(0), _tracker_outputs(1),
    _shift_grid(1), _shift_grid(2),
    Record("inspatio_device.flow_warp", ("inspatio_device.flow_warp",),
           (Arg("grids", "vec", "float32", layout="contiguous", shape=lambda e: (e.N, 4, 4, 2)),
            Arg("has_grid", "vec", layout="contiguous", shape=lambda e: (e.N,)), _frames_in("infilled"), _out()),
           lambda e, a: {"out": mod("inspatio_device").flow_warp(_ctx(e), a["grids"], a["has_grid"], a["infilled"], out=a["out"])},
           (G("grids", "mdvt_flow_warp", 3, row_bytes=lambda e: 128 * e.N, rows=ONE), G("has_grid", "mdvt_flow_warp", 4, row_bytes=lambda e: e.N, rows=ONE),
            G("infilled", "mdvt_flow_warp", 5, 6, 7, 2, R3), G("out", "mdvt_flow_warp", 8, 9, 10, 2, R3))),
    _inspatio_prepare(0), _inspatio_prepare(1),
    Record("inspatio_device.model_frames", ("inspatio_device.model_frames",), (_frames_in(),),
           lambda e, a: {"out": mod("inspatio_device").model_frames(_ctx(e), a["frames"], (e.MW, e.MH))},
           (G("frames", "mdvt_inspatio_model_frames", 3, 4, 5, 2, R3), G("out", "mdvt_inspatio_model_frames", 8, 9, 10, 2, _M3, _MROWS))),
    _inspatio_composite(1, True), _inspatio_composite(0, False),
)

BY_NAME = {r.name: r for r in RECORDS}


# ------------------------------------------------------------------------------------------------------------------------------------
# completeness: the sites of the package's sources
# ------------------------------------------------------------------------------------------------------------------------------------
def pointer_sites(source, module):
    """"<module>.<qualified name>" of every function of a module's source that takes a tensor's address (a `.data_ptr()` call): the
    outermost function, inside its class if it has one -- where a wrapper's nested helper takes it, the wrapper is the site."""
    sites = set()

    def walk(node, path, in_func):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, ast.ClassDef) and not in_func:
                walk(child, path + [child.name], False)
            elif isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)) and not in_func:
                walk(child, path + [child.name], True)
            else:
                if (in_func and isinstance(child, ast.Call) and isinstance(child.func, ast.Attribute) and child.func.attr == "data_ptr"):
                    sites.add(".".join([module] + path))
                walk(child, path, in_func)
    walk(ast.parse(source), [], False)
    return sites


def call_entries(source):
    """The entry points a module's source names in a `.call("mdvt_...", ...)` (a conditional expression of two names gives both)."""
    names = set()
    for node in ast.walk(ast.parse(source)):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "call" and node.args:
            for c in ast.walk(node.args[0]):
                if isinstance(c, ast.Constant) and isinstance(c.value, str) and c.value.startswith("mdvt_"):
                    names.add(c.value)
    return names


def bound_entries(source):
    """The entry points a module's source reaches as an attribute (`..._L.mdvt_render_stereo_batch`: bound past Context.call)."""
    return {n.attr for n in ast.walk(ast.parse(source)) if isinstance(n, ast.Attribute) and n.attr.startswith("mdvt_")}


def package_sites():
    """pointer_sites of every module of the package -> {site: file}."""
    out = {}
    root = os.path.join(REPO, PKG)
    for fn in sorted(os.listdir(root)):
        if fn.endswith(".py"):
            with open(os.path.join(root, fn)) as f:
                for s in pointer_sites(f.read(), fn[:-3]):
                    out[s] = fn
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# building arguments: layouts (passes b and c) and refusal cases (pass a)
# ------------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = ("contiguous", "sbs_right", "sbs_left", "row_pad", "frame_gap", "base_offset", "mid_frame", "expand", "inplace")
GUARD = 64                                   # poisoned elements before and after every buffer


def tdtype(name):
    import torch
    return getattr(torch, name)


def payload(arg, dims, seed):
    """Deterministic content for an argument (a NumPy array of its shape): images with key-coloured and black pixels among random
    ones (holes for the fills, the completion and the blurs), finite positive floats with zeros, small integers."""
    rng = np.random.default_rng([seed, sum(map(ord, arg.name))])
    if arg.dtype == "uint8" and arg.kind == "rgb":
        d = rng.integers(0, 256, dims, dtype=np.uint8)
        pick = rng.random(dims[:-1])
        d[pick < 0.25] = (0, 255, 0)
        d[pick > 0.85] = 0
        return d
    if arg.dtype in ("uint8", "bool"):
        d = (rng.random(dims) < 0.4).astype(np.uint8) * (255 if arg.dtype == "uint8" else 1)
        return d.astype(np.bool_) if arg.dtype == "bool" else d
    if arg.dtype in ("float32", "float64"):
        d = rng.random(dims) * 4 + 0.25
        if arg.kind == "rgb":
            d = d - 2.0                                        # normals: both signs
        elif arg.kind == "plane":
            d[rng.random(dims) < 0.1] = 0.0
        return d.astype(arg.dtype)
    return rng.integers(0, 100, dims).astype(arg.dtype)


class Buffer:
    """One argument as a view into a poisoned storage of its dtype: .t the view the wrapper gets, .store the 1-D storage."""

    def __init__(self, arg, env, layout, seed, device, dtype=None, data=True):
        import torch
        self.arg, self.layout = arg, layout
        dt = tdtype(dtype or arg.dtype)
        dims = arg.dims(env)
        shape, strides, offset, tail, realised = self._geometry(arg, dims, layout)
        self.realised = realised
        span = 1 + sum((s - 1) * st for s, st in zip(shape, strides))
        self.store = torch.empty(2 * GUARD + offset + span + tail, dtype=dt, device=device)
        rng = np.random.default_rng([seed, 99, len(arg.name)])
        nbytes = self.store.numel() * self.store.element_size()
        self.poison = torch.from_numpy(rng.integers(0, 256, nbytes, dtype=np.uint8))
        self.store.view(torch.uint8).copy_(self.poison)
        self.t = self.store.as_strided(shape, strides, GUARD + offset)
        if data:
            dtype_arg = arg if dtype is None else Arg(arg.name, arg.kind, dtype)
            src = torch.from_numpy(payload(dtype_arg, tuple(1 if st == 0 else s for s, st in zip(shape, strides)), seed)).to(device)
            if src.dtype != dt:
                src = src.to(dt)
            self.store.as_strided(tuple(src.shape), strides, GUARD + offset).copy_(src)     # (an expanded batch is written once)
        self.before = None                                     # (pass (c) takes the snapshot: snapshot())

    def snapshot(self):
        self.before = self.bytes()
        return self

    @staticmethod
    def _geometry(arg, dims, layout):
        """(shape, element strides, offset, tail, realised): the view of `dims` in `layout` -- `offset` elements into its storage,
        `tail` more behind it; a layout the argument's promise does not cover (or that does not exist for it) comes out contiguous,
        realised False."""
        dense = [1] * len(dims)
        for k in range(len(dims) - 2, -1, -1):
            dense[k] = dense[k + 1] * dims[k + 1]
        strided = arg.layout in ("strided", "copied") and arg.kind != "vec"
        row = len(dims) - arg.packed - 1 if arg.kind != "vec" else None       # the row dimension (h)
        px = int(np.prod(dims[row + 1:])) if row is not None else 0           # elements per row
        st, off, tail, ok = list(dense), 0, 0, True

        def above(k):
            for j in range(k - 1, -1, -1):
                st[j] = st[j + 1] * dims[j + 1]
        if layout == "contiguous":
            pass
        elif layout == "base_offset":
            off = 1
        elif layout == "mid_frame":               # the middle frame of a batch of three: batch[1:2] (the call's N is 1), or batch[1]
            if arg.kind == "vec" or (arg.batched and dims[0] != 1):
                ok = False
            else:
                off = tail = int(np.prod(dims))
        elif not strided:
            ok = False
        elif layout in ("sbs_right", "sbs_left"):
            st[row] = 2 * px
            above(row)
            off, tail = (px, 0) if layout == "sbs_right" else (0, px)
        elif layout == "row_pad":
            st[row] = px + 5                      # (an odd number of bytes for uint8; of elements for the wider types)
            above(row)
            tail = 5
        elif layout == "frame_gap" and arg.batched and dims[0] > 1:
            st[0] = dense[0] + 7
        elif layout == "expand" and arg.batched and arg.role == "in" and arg.expand and dims[0] > 1:
            st[0] = 0
        else:
            ok = False
        return tuple(dims), tuple(st), off, tail, ok

    def bytes(self):
        import torch
        return self.store.view(torch.uint8).cpu().numpy().copy()

    def owned_mask(self):
        """True at the storage's bytes the view owns."""
        base = self.store.data_ptr()
        m = np.zeros(self.store.numel() * self.store.element_size(), bool)
        m[owned_bytes(self.t) - base] = True
        return m


def layouts_of(record):
    """The layouts pass (b) and (c) run for a record: those at least one of its arguments realises."""
    out = []
    for layout in LAYOUTS:
        if layout == "inplace":
            if record.inplace:
                out.append(layout)
            continue
        if layout == "contiguous":
            out.append(layout)
            continue
        for a in record.args:
            dims = a.dims(Env(8, 4, max(record.min_frames, 1 if layout == "mid_frame" else N_FRAMES)))
            if Buffer._geometry(a, dims, layout)[4]:
                out.append(layout)
                break
    return out


RENDERERS = {}


def close_renderers():
    for r in RENDERERS.values():
        r.close()
    RENDERERS.clear()


def make_env(record, W, H, layout, device=None):
    import torch
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    r = None
    if record.renderer is not None:                                   # one renderer per configuration and size, shared by the passes
        key = (tuple(sorted(record.renderer.items())), W, H)
        if key not in RENDERERS:
            RENDERERS[key] = mod("stereo_rerender").StereoRerenderer(W, H, **record.renderer)
        r = RENDERERS[key]
    env = Env(W, H, max(record.min_frames, 1 if layout == "mid_frame" else N_FRAMES), device, r)
    if record.setup:
        record.setup(env)
    return env


def build_args(record, env, layout, seed=1, outputs=True, alt_dtypes=False):
    """{name: Buffer} for a record in a layout.  outputs False: the optional outputs are left out (out=None); alt_dtypes: the
    arguments whose docstring allows a second dtype (a bool mask) come in that one."""
    bufs = {}
    for a in record.args:
        if a.role == "out" and a.optional and not outputs:
            continue
        lay = "contiguous" if layout == "inplace" else layout
        bufs[a.name] = Buffer(a, env, lay, seed, env.device, dtype=a.also[0] if alt_dtypes and a.also else None)
    if layout == "inplace":
        src, dst = record.inplace
        bufs[dst] = bufs[src]
    return bufs


def tensors(record, bufs):
    return {a.name: (bufs[a.name].t if a.name in bufs else None) for a in record.args}


def resolve(spec, call, env):
    if isinstance(spec, tuple) and spec and spec[0] == "=":
        return spec[1]
    if spec is None:
        return None
    if isinstance(spec, str):
        io = next(a for a in call.args if isinstance(a, dict) and spec in a)
        return io[spec] or 0
    return call.args[spec]


def touches_of(record, calls, env):
    """{argument or result name: [Touch, ...]} of a record's groups over the recorded calls."""
    out = {}
    for g in record.groups:
        for c in calls:
            if c.name != g.entry:
                continue
            ptr = resolve(g.ptr, c, env)
            rb, rows = int(g.row_bytes(env)), int(g.rows(env))
            pitch = resolve(g.pitch, c, env)
            stride = resolve(g.stride, c, env)
            n = int(resolve(g.n, c, env))
            out.setdefault(g.arg, []).append(Touch(int(ptr or 0) + int(g.offset(env)), int(rb if pitch is None else pitch),
                                                   int(0 if stride is None else stride), n, rb, rows, g.planes, int(resolve(g.plane, c, env) or 0)))
    return out


def geometry_problems(record, env, layout, seed=1, alt_dtypes=False):
    """Pass (b) for one record and layout: record the call, hold every pointer group to its tensor's own bytes.  Launches nothing."""
    bufs = build_args(record, env, layout, seed, alt_dtypes=alt_dtypes)
    a = tensors(record, bufs)
    with Recorder() as rec:
        env.recorder = rec
        try:
            results = record.call(env, a)
        finally:
            env.recorder = None
    problems = []
    if not rec.calls:
        return [f"{record.name} [{layout}]: no library call was recorded"]
    touched = touches_of(record, rec.calls, env)
    for g_arg in dict.fromkeys(g.arg for g in record.groups):
        what = f"{record.name} [{layout}{', second dtype' if alt_dtypes else ''}, {env.W}x{env.H}] {g_arg}"
        groups = [g for g in record.groups if g.arg == g_arg]
        ts = touched.get(g_arg, [])
        spec = next((x for x in record.args if x.name == g_arg), None)
        t = a.get(g_arg)
        if t is None:
            t = results.get(g_arg)
        if t is None:
            problems.append(f"{what}: neither an argument nor a result")
            continue
        output = spec is None or spec.role == "out"
        if spec is not None and spec.layout == "copied":
            # the wrapper's contiguous copy: dense rows of the argument's size, outside the caller's storage
            for k in ts if not (ts and ts[0].ptr == t.data_ptr()) else ():
                if k.pitch != k.row_bytes or (k.n > 1 and k.stride != k.rows * k.pitch):
                    problems.append(f"{what}: the recorded geometry is not that of a contiguous copy (pitch {k.pitch}, stride {k.stride} for "
                                    f"{k.rows} rows of {k.row_bytes} bytes)")
            if ts and ts[0].ptr == t.data_ptr():              # not copied: then the geometry must be the argument's own
                problems += check_groups(what, t, ts, output, any(g.partial for g in groups))
            elif ts and np.isin(ts[0].addresses(), owned_bytes(bufs[g_arg].store)).any():
                problems.append(f"{what}: the copy's address lies inside the caller's storage")
            continue
        problems += check_groups(what, t, ts, output, any(g.partial for g in groups))
    return problems


def same_bits(x, y):
    """Equality of bytes; for floats: the same bits, or both NaN."""
    import torch
    if isinstance(x, torch.Tensor):
        if not isinstance(y, torch.Tensor) or x.shape != y.shape or x.dtype != y.dtype:
            return False
        xa, ya = x.detach().cpu().contiguous().numpy(), y.detach().cpu().contiguous().numpy()
        if xa.dtype.kind == "f":
            return bool(np.all((xa.view(f"u{xa.itemsize}") == ya.view(f"u{ya.itemsize}")) | (np.isnan(xa) & np.isnan(ya))))
        return bool(np.array_equal(xa, ya))
    if isinstance(x, np.ndarray):
        return isinstance(y, np.ndarray) and np.array_equal(x, y)
    return x == y


def result_problems(record, env, layout, seed=1, alt_dtypes=False):
    """Pass (c) for one record and layout that passed (b): launch on the views, launch on contiguous copies with out=None, compare."""
    bufs = build_args(record, env, layout, seed, alt_dtypes=alt_dtypes)
    for b in bufs.values():
        b.snapshot()
    a = tensors(record, bufs)
    got = record.call(env, a)
    import torch
    torch.cuda.synchronize()
    problems = []
    what = f"{record.name} [{layout}, {env.W}x{env.H}]"
    # the reference run: contiguous copies of the same content, out=None (a required output: a contiguous tensor of the same content)
    ref_bufs = build_args(record, env, "contiguous", seed, outputs=False)
    for x in record.args:                                              # (same content whatever the layout: an expanded batch repeats its frame)
        if x.role == "in" or not x.optional:
            ref_bufs[x.name] = _contiguous_copy(x, env, bufs[x.name])
    want = record.call(env, tensors(record, ref_bufs))
    torch.cuda.synchronize()
    for k in want:
        if k not in got or not same_bits(got[k], want[k]):
            problems.append(f"{what}: result '{k}' read through the view differs from the contiguous call's")
    outs = {x.name for x in record.args if x.role == "out"}
    done = set()
    for name, b in bufs.items():
        if id(b) in done:
            continue
        done.add(id(b))
        after = b.bytes()
        is_out = name in outs or (layout == "inplace" and record.inplace and name in record.inplace)
        keep = ~b.owned_mask() if is_out else np.ones(after.size, bool)
        changed = np.nonzero((after != b.before) & keep)[0]
        if changed.size:
            problems.append(f"{what}: {changed.size} byte(s) of {'the padding and gaps of output' if is_out else 'input'} '{name}' changed, "
                            f"the first at byte {int(changed[0])} of its storage")
    return problems


def _contiguous_copy(arg, env, buf):
    """A contiguous Buffer holding what `buf`'s view held before the call."""
    import torch
    c = Buffer(arg, env, "contiguous", 5, env.device, dtype=str(buf.store.dtype).split(".")[-1], data=False)
    before = torch.from_numpy(buf.before).to(env.device).view(buf.store.dtype)
    c.t.copy_(before.as_strided(tuple(buf.t.shape), tuple(buf.t.stride()), buf.t.storage_offset()))
    return c.snapshot()


# ------------------------------------------------------------------------------------------------------------------------------------
# pass (a): the refusals
# ------------------------------------------------------------------------------------------------------------------------------------
WRONG_DTYPES = {"uint8": ("int8", "int32", "float32", "bool"), "float32": ("float64", "float16"), "float64": ("float32",), "int64": ("int32",),
                "bool": ("float32",)}


def refusal_cases(record, arg, env):
    """[(case name, tensor)] every one of which the wrapper must refuse for `arg` (the other arguments are good and contiguous)."""
    import torch
    dev = env.device
    dims = arg.dims(env)
    dt = tdtype(arg.dtype)

    def full(shape, dtype=dt, device=dev):
        return torch.zeros(tuple(shape), dtype=dtype, device=device)

    cases = []
    for wrong in WRONG_DTYPES[arg.dtype]:
        if wrong not in arg.also:
            cases.append((f"dtype {wrong}", full(dims, tdtype(wrong))))
    cases.append(("a CPU tensor", full(dims, device="cpu")))
    if torch.cuda.device_count() >= 2:
        other = torch.device("cuda", (torch.device(dev).index or torch.cuda.current_device()) ^ 1)
        cases.append(("a tensor on the other GPU", full(dims, device=other)))
    if arg.kind == "vec":
        cases.append(("one row too few", full((max(dims[0] - 1, 0),) + tuple(dims[1:]))))
        if len(dims) == 2:
            cases.append(("non-contiguous", full((dims[0], 2 * dims[1]))[:, ::2]))
        return cases
    row = len(dims) - arg.packed - 1
    sized = ((not arg.leads) or arg.fixed) and not arg.free_hw

    def bump(k, by):
        d = list(dims)
        d[k] += by
        return tuple(d)
    if sized:
        cases.append(("wrong H", full(bump(row, 1))))
        cases.append(("wrong W", full(bump(row + 1, 2 if arg.wide == 2 else 1))))
    if arg.batched and not arg.leads and not arg.fewer_ok:
        cases.append(("fewer frames than N", full(bump(0, -1))))
    if arg.batched and arg.role == "in" and arg.expand is False and dims[0] > 1:
        cases.append(("overlapping frames: expand", full((1,) + tuple(dims[1:])).expand(dims)))
    if arg.layout != "copied":
        if arg.kind == "rgb":
            cases.append(("unpacked pixels rgba[..., :3]", full(dims[:-1] + (4,))[..., :3]))
            cases.append(("unpacked pixels img[:, ::2]", full(bump(row + 1, dims[row + 1]))[..., ::2, :]))
        else:
            cases.append(("unpacked pixels p[:, ::2]", full(bump(row + 1, dims[row + 1]))[..., ::2]))
        if dims[row] == dims[row + 1]:
            cases.append(("the transposed square view", full(dims).transpose(row, row + 1)))
    if arg.layout == "contiguous":
        cases.append(("non-contiguous: padded rows", full(bump(row + 1, 1))[..., :-1, :] if arg.kind == "rgb" else full(bump(row + 1, 1))[..., :-1]))
        cases.append(("non-contiguous: one eye of a side-by-side buffer",
                      full(bump(row + 1, dims[row + 1]))[..., dims[row + 1]:, :] if arg.kind == "rgb" else full(bump(row + 1, dims[row + 1]))[..., dims[row + 1]:]))
        if arg.batched and dims[0] > 1:
            cases.append(("non-contiguous: every other frame", full(bump(0, dims[0]))[::2]))
    if arg.role == "out":
        if arg.batched and dims[0] > 1:
            cases.append(("overlapping: expand", full((1,) + tuple(dims[1:])).expand(dims)))
        cases.append(("overlapping: expanded rows", full(dims[:row] + (1,) + dims[row + 1:]).expand(dims)))
        st = list(full(dims).stride())
        st[row] = max(st[row] - 2, 1)
        for k in range(row - 1, -1, -1):
            st[k] = st[k + 1] * dims[k + 1]
        cases.append(("overlapping: as_strided with a pitch below the row", torch.as_strided(full((int(np.prod(dims)) + 8,)), dims, st)))
    return cases


def refusal_problems(record, env, seed=1):
    """Pass (a) for one record: every bad tensor for every tensor argument, with the recorder installed.  Launches nothing: a case
    that is not refused shows as a recorded call (or a clean return), never as a kernel on a bad address."""
    problems = []
    good = tensors(record, build_args(record, env, "contiguous", seed))
    for arg in record.args:
        for case, bad in refusal_cases(record, arg, env):
            a = dict(good)
            a[arg.name] = bad
            outcome = None
            with Recorder() as rec:
                env.recorder = rec
                try:
                    record.call(env, a)
                    outcome = "was accepted"
                except (TypeError, ValueError):
                    pass
                except AssertionError:
                    outcome = "was refused by an assert, which python -O strips"
                except Exception as e:                                  # noqa: BLE001
                    outcome = f"raised {type(e).__name__} ({e}), not the TypeError / ValueError of a refusal"
                finally:
                    env.recorder = None
            if rec.calls:
                problems.append(f"{record.name}({arg.name}: {case}): {len(rec.calls)} call(s) reached the library, the first {rec.calls[0].name}")
            elif outcome:
                problems.append(f"{record.name}({arg.name}: {case}) {outcome}")
    return problems
