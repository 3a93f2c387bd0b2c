"""What the entry points of csrc/mdvt_api.hip (and the two of csrc/mdvt_api_render.hip whose checks have the same form) answer to wrong arguments: status and mdvt_last_error text, pinned character for
character.  Python callers read these texts inside MdvtError, and the order of an entry point's checks decides which one they get.

TABLE holds one small valid call per entry point, as a list of typed arguments in the order of the C declaration (frames of 8 to
16 pixels a side, n = 2).  The wrong calls are generated from it by argument kind:

    ptr      -> NULL                            pitch  -> one byte below its row       stride -> one byte below its frame
    count    -> 0 and -1                        size   -> 0 (unsigned: nothing is smaller)
    flag     -> 2 and -1                        depth  -> 0.0, NaN and -1.0 (a double that has to be positive)
    val      -> not mutated (test_refusal_cases_cpu.py wants a reason for each)

then the entry's `extra` cases (the "too large" and alignment refusals, reached with argument values alone: nothing large is
allocated, and each is refused by a check that no other argument switches off), then every pair of consecutive cases with both
arguments wrong.  A mutation only makes a value smaller, NULL or out of range, so a call the library accepts stays inside its
buffers: an optional pointer's NULL is accepted, and recorded as accepted like any other result.

All device pointers point into one uint8 tensor, each argument into a region of its own with MARGIN bytes on either side.
tests/test_gpu_refusal_text.py runs the cases and compares them with tests/golden/refusal_text.json;
`python tests/refusal_cases.py --record` writes that file (it was recorded with the library of the commit BEFORE this
module was added, and has to stay as it is whenever csrc/ is only tidied).  Plain module: no fixture, no pytest
setting."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "refusal_text.json")
for _p in (REPO, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

W, H, N = 12, 8, 2                               # the context's size (and most entry points' own), frames per call
MARGIN = 1024                                    # bytes around every argument's region
ROW = 3 * W                                      # a u8 RGB row
FFV1_CASE = (W, H, N, 1, 1, 1, 1, (2, 1))        # tests/ffv1_streams.py: intra-only range-coder frames, both decoders' class


class Arg:
    def __init__(self, kind, name, value=None, ctype=None, fill=None):
        self.kind, self.name, self.value, self.ctype, self.fill = kind, name, value, ctype, fill

    def __repr__(self):
        return f"{self.kind}:{self.name}"


def ctx():
    return Arg("ctx", "ctx")


def stream():
    return Arg("stream", "stream")


def ptr(name, nbytes, fill=None):
    """A device pointer to a region of nbytes (zeros, or what fill(data) returns: bytes)."""
    return Arg("ptr", name, int(nbytes), fill=fill)


def host(name, what):
    """A host pointer: what = "config" / "packet" (bytes of the FFV1 fixture), "params" (N frames' mdvt_frame_params) or a count
    of floats."""
    return Arg("host", name, what)


def pitch(name, row):
    return Arg("pitch", name, int(row), C.c_size_t)


def stride(name, frame):
    return Arg("stride", name, int(frame), C.c_size_t)


def count(name, v):
    return Arg("count", name, int(v), C.c_int)


def size(name, v, ctype=C.c_uint64):
    return Arg("size", name, v, ctype)


def flag(name, v=0):
    return Arg("flag", name, int(v), C.c_int)


def depth(name, v):
    return Arg("depth", name, float(v), C.c_double)


def val(name, ctype, v):
    return Arg("val", name, v, ctype)


class Entry:
    def __init__(self, name, args, extra=(), returns="status", needs_config=False):
        self.name, self.args, self.extra, self.returns, self.needs_config = name, list(args), list(extra), returns, needs_config
        self.by_name = {a.name: a for a in self.args}
        assert len(self.by_name) == len(self.args), name

    def cases(self):
        """[(label, {argument: wrong value})] in the order of the arguments, then the extra cases."""
        out = []
        for a in self.args:
            if a.kind in ("ptr", "host"):
                out.append((f"{a.name} NULL", {a.name: None}))
            elif a.kind in ("pitch", "stride"):
                out.append((f"{a.name} one byte short", {a.name: a.value - 1}))
            elif a.kind == "count":
                out += [(f"{a.name} 0", {a.name: 0}), (f"{a.name} -1", {a.name: -1})]
            elif a.kind == "size":
                out.append((f"{a.name} 0", {a.name: 0}))
            elif a.kind == "flag":
                out += [(f"{a.name} 2", {a.name: 2}), (f"{a.name} -1", {a.name: -1})]
            elif a.kind == "depth":
                out += [(f"{a.name} 0.0", {a.name: 0.0}), (f"{a.name} NaN", {a.name: math.nan}), (f"{a.name} -1.0", {a.name: -1.0})]
        return out + [(label, dict(wrong)) for label, wrong in self.extra]

    def all_cases(self):
        """The valid call, every case, and every pair of consecutive cases with both arguments wrong (the later one's value where
        both name the same argument)."""
        single = self.cases()
        out = [("valid", {})] + single
        for (la, wa), (lb, wb) in zip(single, single[1:]):
            out.append((f"{la} + {lb}", {**wa, **wb}))
        return out

    def mutated(self):
        """The arguments some case gives a wrong value."""
        return {k for _, wrong in self.cases() for k in wrong}


class Misaligned:
    """An extra case's pointer value: the argument's own region, `by` bytes in (inside its margin)."""

    def __init__(self, by=1):
        self.by = by


def _rgb(n=N, w=W, h=H):
    return 3 * w * h * n


# ---- the FFV1 fixture: packets one behind the other, their offsets and sizes -------------------------------------------------
def ffv1_fixture():
    import numpy as np
    import ffv1_streams as fs
    _, packets, config = fs.make_stream(FFV1_CASE)
    sizes = np.array([len(p) for p in packets], np.uint32)
    offsets = np.concatenate([[0], np.cumsum(sizes[:-1])]).astype(np.uint64)
    return dict(config=bytes(config), packet=bytes(packets[0]), blob=b"".join(packets), offsets=offsets.tobytes(), sizes=sizes.tobytes())


BLOB_CAP = 8192                                  # room for the fixture's packets, and the encoder's packets_cap


def _decoder_args(n_name):
    return [ctx(), count("width", W), count("height", H), host("h_config", "config"), size("config_size", "config", C.c_size_t),
            ptr("d_packets", BLOB_CAP, fill="blob"), size("packets_bytes", "blob"), ptr("d_offsets", 8 * N, fill="offsets"),
            ptr("d_sizes", 4 * N, fill="sizes"), count(n_name, N)]


def _decoder_tail():
    return [ptr("d_dst", _rgb()), pitch("pitch", ROW), stride("frame_stride", ROW * H), flag("order"), ptr("d_status", 4 * N), stream()]


_BIG_W, _BIG_H = 1 << 15, 1 << 14                # 2^29 pixels: past the 2^28 of the FFV1 units and the convergence depths
_BIG_FRAME = dict(width=_BIG_W, height=_BIG_H, pitch=3 * _BIG_W, frame_stride=3 * _BIG_W * _BIG_H)
_OUT_2_31 = dict(out_w=1 << 16, out_h=1 << 15, codes_pitch=3 << 16, codes_stride=3 << 31)      # test_gpu_depth_sink_footprint.py's
TALL = 65536                                     # one row more than a grid dimension holds

# the side-by-side colour and mask frames of the adapter calls (two eyes of EW x EH), the model's frames, m2svid's other sizes
EW, EH, MW, MH = 12, 8, 10, 9
OW_, OH_, KW, KH = 14, 6, 5, 4
SBS = 6 * EW


def _sbs(name, pname=None):
    pname = pname or name[2:]
    return [ptr(name, SBS * EH * N), pitch(f"{pname}_pitch", SBS), stride(f"{pname}_stride", SBS * EH)]


def _plane(name, row, rows, pname=None, n=N):
    pname = pname or name[2:]
    return [ptr(name, row * rows * n), pitch(f"{pname}_pitch", row), stride(f"{pname}_stride", row * rows)]


def _finish(stereo, heap):
    seed = [ptr("d_left_seed", _rgb()), ptr("d_right_seed", _rgb())] if stereo else [ptr("d_seed", _rgb())]
    out = [ptr("d_left_out", _rgb()), ptr("d_right_out", _rgb())] if stereo else [ptr("d_out", _rgb())]
    n = count("n_frames" if stereo else "n_images", N)
    rounds = [] if heap else [count("max_rounds", 8)]
    return ([ctx()] + seed + [pitch("seed_pitch", ROW), stride("seed_stride", ROW * H)] + out + [pitch("out_pitch", ROW), stride("out_stride", ROW * H), n]
            + rounds + [ptr("d_remaining", 4 * N * (2 if stereo else 1)), stream()])


_ROUNDS = [("max_rounds 32767", dict(max_rounds=32767)), ("max_rounds -32767", dict(max_rounds=-32767))]
_MARCH = 1 << 24                                 # the first pitch the march's 24-bit multiply cannot hold

TABLE = [
    Entry("mdvt_decode_depth", [ctx(), ptr("d_rgb", _rgb(1)), pitch("rgb_pitch", ROW), ptr("d_depth", 4 * W * H), pitch("depth_pitch", 4 * W),
                                depth("max_depth", 20.0), val("depth_scale", C.c_double, 1.0), stream()]),
    Entry("mdvt_encode_depth", [ctx(), ptr("d_depth", 4 * W * H), pitch("depth_pitch", 4 * W), ptr("d_rgb", _rgb(1)), pitch("rgb_pitch", ROW),
                                depth("max_depth", 20.0), flag("bgr"), stream()]),
    Entry("mdvt_infill_using_normals",
          [ctx(), ptr("d_color", _rgb(1)), pitch("color_pitch", ROW), ptr("d_hole", W * H), pitch("hole_pitch", W), ptr("d_normal", 12 * W * H),
           pitch("normal_pitch", 12 * W), ptr("d_out", _rgb(1)), pitch("out_pitch", ROW), count("max_steps", 4), stream()],
          extra=[("hole_pitch 2^24", dict(hole_pitch=_MARCH))]),
    Entry("mdvt_mark_lower_side", [ctx(), ptr("d_normals_img", _rgb(1)), pitch("img_pitch", ROW), ptr("d_out", _rgb(1)), pitch("out_pitch", ROW),
                                   count("max_steps", 4), stream()],
          extra=[("img_pitch 2^24", dict(img_pitch=_MARCH))]),
    Entry("mdvt_touchly_depth", [ctx(), ptr("d_depth", 4 * W * H), pitch("depth_pitch", 4 * W), ptr("d_rgb", _rgb(1)), pitch("rgb_pitch", ROW),
                                 depth("touchly_max_depth", 10.0), depth("touchly_min_depth", 0.5), flag("zero_is_far"), stream()]),
    Entry("mdvt_equirect_tables", [count("width", W), count("height", H), depth("input_fov_deg", 90.0), host("h_map_x", W), host("h_map_y", H)]),
    Entry("mdvt_equirect_remap", [ctx(), ptr("d_src", _rgb()), pitch("src_pitch", ROW), stride("src_stride", ROW * H), ptr("d_dst", _rgb()),
                                  pitch("dst_pitch", ROW), stride("dst_stride", ROW * H), count("n_images", N), ptr("d_map_x", 4 * W),
                                  ptr("d_map_y", 4 * H), stream()]),
    Entry("mdvt_swap_rb", [ctx(), ptr("d_src", _rgb()), pitch("src_pitch", ROW), stride("src_stride", ROW * H), ptr("d_dst", _rgb()),
                           pitch("dst_pitch", ROW), stride("dst_stride", ROW * H), count("n_images", N), stream()]),
    Entry("mdvt_masked_blur", [ctx(), ptr("d_img", _rgb(1)), pitch("img_pitch", ROW), ptr("d_out", _rgb(1)), pitch("out_pitch", ROW), stream()]),
    Entry("mdvt_normal_infill", [ctx()] + _plane("d_img", ROW, H) + _plane("d_infill_mask", ROW, H, "mask") + _plane("d_out", ROW, H)
          + [count("n_images", N), stream()],
          extra=[("mask_pitch 2^24", dict(mask_pitch=_MARCH))]),
    Entry("mdvt_infill_using_mask_normals", [ctx()] + _plane("d_img", ROW, H) + _plane("d_hole", W, H) + _plane("d_mask_img", ROW, H, "mask")
          + [count("n_images", N), count("max_steps", 4), stream()],
          extra=[("hole_pitch 2^24", dict(hole_pitch=_MARCH))]),
    Entry("mdvt_finish_infill_mask_heap", _finish(False, True)),
    Entry("mdvt_finish_infill_mask_heap_stereo", _finish(True, True)),
    Entry("mdvt_finish_infill_mask", _finish(False, False), extra=_ROUNDS),
    Entry("mdvt_finish_infill_mask_stereo", _finish(True, False), extra=_ROUNDS),
    Entry("mdvt_encode_video_frames",
          [ctx(), count("width", W), count("height", H), count("slices_h", 2), count("slices_v", 1), ptr("d_src", _rgb()), pitch("pitch", ROW),
           stride("frame_stride", ROW * H), count("channels", 3), flag("order"), count("n_frames", N), val("slice_capacity", C.c_uint64, 0),
           ptr("d_packets", BLOB_CAP), size("packets_cap", BLOB_CAP), ptr("d_offsets", 8 * N), ptr("d_sizes", 4 * N), stream()],
          extra=[("2^29 pixels", _BIG_FRAME), ("1025 slices", dict(slices_h=41, slices_v=25, width=41, height=25, pitch=123,
                                                                     frame_stride=123 * 25))]),
    Entry("mdvt_ffv1_decode_supported", [host("h_config", "config"), size("config_size", "config", C.c_size_t)], returns="text"),
    Entry("mdvt_ffv1_stream_decode_supported", [host("h_config", "config"), size("config_size", "config", C.c_size_t)], returns="text"),
    Entry("mdvt_ffv1_packet_is_key", [host("h_packet", "packet"), size("size", "packet", C.c_size_t)], returns="value"),
    Entry("mdvt_decode_video_frames", _decoder_args("n_frames") + _decoder_tail(), extra=[("2^29 pixels", _BIG_FRAME)]),
    Entry("mdvt_decode_video_stream", _decoder_args("n_packets") + [count("first_out", 0)] + _decoder_tail(),
          extra=[("first_out = n_packets", dict(first_out=N)), ("2^29 pixels", _BIG_FRAME), ("2^29 packets", dict(n_packets=1 << 29))]),
    Entry("mdvt_convergence_depths",
          [ctx(), count("width", W), count("height", H)] + _plane("d_depth", ROW, H) + [flag("depth_order")] + _plane("d_mask", ROW, H)
          + [flag("mask_order"), count("n_frames", N), count("n_mask_frames", N), depth("max_depth", 20.0), ptr("d_means", 4 * N),
             ptr("d_counts", 4 * N), stream()],
          extra=[("more mask frames than frames", dict(n_mask_frames=N + 1)),
                 ("2^29 pixels", dict(width=_BIG_W, height=_BIG_H, depth_pitch=3 * _BIG_W, depth_stride=3 * _BIG_W * _BIG_H, mask_pitch=3 * _BIG_W,
                                      mask_stride=3 * _BIG_W * _BIG_H))]),
    Entry("mdvt_scale_shift_fit",
          [ctx(), count("width", W), count("height", H), count("n_frames", N)] + _plane("d_pred", 4 * W, H) + _plane("d_target", 4 * W, H)
          + [flag("target_is_depth")] + _plane("d_mask", W, H) + [ptr("d_out", 32), stream()],
          extra=[("2^31 values", dict(width=1 << 16, height=1 << 15, pred_pitch=4 << 16, pred_stride=4 << 31, target_pitch=4 << 16,
                                      target_stride=4 << 31, mask_pitch=1 << 16, mask_stride=1 << 31))]),
    Entry("mdvt_metric_depth_codes",
          [ctx(), count("in_w", W), count("in_h", H), count("n_frames", N)] + _plane("d_rel", 4 * W, H) + [ptr("d_scale_shift", 8), flag("style"),
           depth("max_depth", 20.0), count("out_w", 16), count("out_h", 10)] + _plane("d_codes", 48, 10) + [flag("order")] + _plane("d_depth", 64, 10)
          + [stream()],
          extra=[("2^31 pixels", dict(_OUT_2_31, depth_pitch=4 << 16, depth_stride=4 << 31))]),
    Entry("mdvt_depth_video_codes",
          [ctx(), count("in_w", W), count("in_h", H), count("n_frames", N)] + _plane("d_depth", 4 * W, H) + [ptr("d_scale", 4), flag("nan_to_max"),
           depth("max_depth", 20.0), count("out_w", 16), count("out_h", 10)] + _plane("d_codes", 48, 10) + [flag("order")] + _plane("d_plane", 64, 10)
          + [stream()],
          extra=[("2^31 pixels", dict(_OUT_2_31, plane_pitch=4 << 16, plane_stride=4 << 31))]),
    Entry("mdvt_adapter_prepare_eye",
          [ctx(), count("eye_w", EW), count("eye_h", EH), count("n_frames", N), flag("eye")] + _sbs("d_color") + _sbs("d_mask")
          + [count("model_w", MW), count("model_h", MH)] + _plane("d_image", 3 * MW, MH) + _plane("d_model_mask", MW, MH)
          + [ptr("d_hole_counts", 4 * N), stream()],
          extra=[("d_hole_counts misaligned", dict(d_hole_counts=Misaligned())),
                 ("model_h 65536", dict(model_h=TALL, image_stride=3 * MW * TALL, model_mask_stride=MW * TALL))]),
    Entry("mdvt_lhm_moments",
          [ctx(), count("width", W), count("height", H), count("n_frames", N), ptr("d_rgb", _rgb()), pitch("pitch", ROW), stride("stride", ROW * H)]
          + _plane("d_mask", W, H) + [ptr("d_out", 80 * N), stream()],
          extra=[("d_out misaligned", dict(d_out=Misaligned(4)))]),
    Entry("mdvt_lhm_apply",
          [ctx(), count("width", W), count("height", H), count("n_frames", N), ptr("d_rgb", _rgb()), pitch("pitch", ROW), stride("stride", ROW * H),
           ptr("d_params", 120 * N)] + _plane("d_out", ROW, H) + [stream()],
          extra=[("d_params misaligned", dict(d_params=Misaligned(4))), ("height 65536", dict(height=TALL, stride=ROW * TALL, out_stride=ROW * TALL))]),
    Entry("mdvt_adapter_composite_eye",
          [ctx(), count("eye_w", EW), count("eye_h", EH), count("n_frames", N), flag("eye"), ptr("d_model", 3 * MW * MH * N), count("model_w", MW),
           count("model_h", MH), pitch("model_pitch", 3 * MW), stride("model_stride", 3 * MW * MH)] + _sbs("d_color") + _sbs("d_mask")
          + _sbs("d_pasted") + _sbs("d_blended") + [stream()],
          extra=[("eye 7 x 7", dict(eye_w=7, eye_h=7)),
                 ("eye_h 65536", dict(eye_h=TALL, color_stride=SBS * TALL, mask_stride=SBS * TALL, pasted_stride=SBS * TALL, blended_stride=SBS * TALL)),
                 ("mask_pitch 2^24", dict(mask_pitch=_MARCH, mask_stride=_MARCH * EH))]),
    Entry("mdvt_m2svid_prepare_eye",
          [ctx(), count("eye_w", EW), count("eye_h", EH), count("n_frames", N), flag("eye")] + _sbs("d_color") + _sbs("d_mask")
          + [ptr("d_org", 3 * OW_ * OH_ * N), count("org_w", OW_), count("org_h", OH_), pitch("org_pitch", 3 * OW_), stride("org_stride", 3 * OW_ * OH_),
             count("image_w", MW), count("image_h", MH), count("mask_w", KW), count("mask_h", KH)]
          + _plane("d_image", 3 * MW, MH) + _plane("d_org_image", 3 * MW, MH) + _plane("d_model_mask", KW, KH) + [ptr("d_hole_counts", 4 * N), stream()],
          extra=[("d_hole_counts misaligned", dict(d_hole_counts=Misaligned())),
                 ("image_h 65536", dict(image_h=TALL, image_stride=3 * MW * TALL, org_image_stride=3 * MW * TALL)),
                 ("mask_h 65536", dict(mask_h=TALL, model_mask_stride=KW * TALL))]),
    Entry("mdvt_model_infill_finish",
          [ctx(), count("width", W), count("height", H), count("n_images", N)] + _plane("d_img", ROW, H) + _plane("d_model", ROW, H)
          + _plane("d_infill_mask", ROW, H, "mask") + _plane("d_out", ROW, H) + [stream()],
          extra=[("mask_pitch 2^24", dict(mask_pitch=_MARCH, mask_stride=_MARCH * H)),
                 ("height 65536", dict(height=TALL, img_stride=ROW * TALL, model_stride=ROW * TALL, mask_stride=ROW * TALL, out_stride=ROW * TALL))]),
    # csrc/mdvt_api_render.hip: the two entry points there whose checks have the forms of mdvt_api.hip's (plain arguments, no struct)
    Entry("mdvt_depth_grey_batch",
          [ctx(), count("n_frames", N), ptr("d_depth_rgb", _rgb()), pitch("pitch", ROW), stride("stride", ROW * H), depth("max_depth", 20.0),
           count("bits", 8)] + _plane("d_out", ROW, H) + [stream()],
          extra=[("16 bits, d_out misaligned", dict(bits=16, d_out=Misaligned()))]),
    Entry("mdvt_view_centers",
          [ctx(), count("n_frames", N), host("params", "params"), ptr("d_depth_rgb", _rgb()), pitch("depth_pitch", ROW), stride("depth_stride", ROW * H),
           ptr("d_centers", 64 * N), stream()],
          extra=[("d_centers misaligned", dict(d_centers=Misaligned(4)))], needs_config=True),
]
RENDER_UNIT = ("mdvt_depth_grey_batch", "mdvt_view_centers")

BY_NAME = {e.name: e for e in TABLE}

# Parameters no case mutates -> why.  The two admissible reasons: the header refuses no value of the parameter that a test can
# pass, or the refusal needs an allocation failure or a HIP error.
NO_VALUE_REFUSED = "the header refuses no value of the parameter"
EXEMPT = {
    ("mdvt_decode_depth", "depth_scale"): NO_VALUE_REFUSED + ": any double scales the depth",
    ("mdvt_encode_video_frames", "slice_capacity"): NO_VALUE_REFUSED + ": 0 is the default, a small one flags the frame in d_sizes",
}
for _e in TABLE:
    if _e.by_name.get("stream"):
        EXEMPT[(_e.name, "stream")] = NO_VALUE_REFUSED + ": any stream handle, NULL included, is taken as it is"


def layout():
    """{(entry, argument): offset of the region in the one buffer}, total bytes.  Every region starts on a 256-byte boundary and
    has MARGIN bytes before and after it that belong to no other region."""
    at, off = {}, MARGIN
    for e in TABLE:
        for a in e.args:
            if a.kind == "ptr":
                off = (off + 255) & ~255
                at[(e.name, a.name)] = off
                off += a.value + 2 * MARGIN
    return at, off


def arguments(e, wrong, base, at, handle, fixture, keep):
    """The ctypes arguments of entry e's call with the values of `wrong` put in.  keep: a list that holds the host buffers alive."""
    out = []
    for a in e.args:
        v = wrong.get(a.name, a.value)
        if a.kind == "ctx":
            out.append(handle)
        elif a.kind == "stream":
            out.append(None)
        elif a.kind == "ptr":
            here = base + at[(e.name, a.name)]
            if a.name in wrong:
                out.append(None if v is None else C.c_void_p(here + v.by))
            else:
                out.append(C.c_void_p(here))
        elif a.kind == "host":
            if a.name in wrong:
                out.append(None)
            elif isinstance(a.value, str):
                out.append(fixture[a.value])
            else:
                keep.append((C.c_float * a.value)())
                out.append(keep[-1])
        elif a.kind == "size" and isinstance(v, str):
            out.append(len(fixture[v]))
        else:
            out.append(v)
    return out


def frame_params(_lib):
    """N frames' parameters of a plain camera of the context's size."""
    arr = (_lib.MdvtFrameParams * N)()
    for p in arr:
        for k, v in enumerate((10.0, 0.0, W / 2, 0.0, 10.0, H / 2, 0.0, 0.0, 1.0)):
            p.K[k] = p.Krender[k] = v
        p.depth_scale = 1.0
    return arr


def run_all(device=0):
    """Every case of every entry point on the loaded library -> {entry: {label: [status, text]}}.  Needs a GPU.  `status` of the two
    *_supported calls: 0 = supported (they return the text itself, or NULL); the text of an accepted call is ""."""
    import numpy as np
    import torch
    from metric_depth_video_toolbox_amd import _lib
    torch.cuda.init()
    L = _lib.load()
    fixture = dict(ffv1_fixture(), params=frame_params(_lib))
    assert len(fixture["blob"]) <= BLOB_CAP
    at, total = layout()
    hostbuf = np.zeros(total, np.uint8)
    for e in TABLE:
        for a in e.args:
            if a.kind == "ptr" and a.fill:
                data = np.frombuffer(fixture[a.fill], np.uint8)
                hostbuf[at[(e.name, a.name)]: at[(e.name, a.name)] + data.size] = data
    pristine = torch.from_numpy(hostbuf).to(f"cuda:{device}")
    buf = pristine.clone()
    base = buf.data_ptr()
    assert base % 256 == 0
    ctx_ = _lib.Context(device, W, H)
    res = {}
    try:
        for e in TABLE:
            fn = getattr(L, e.name)
            if e.needs_config:                   # (from here on: no entry point before this one sees a configuration)
                cfg = _lib.MdvtConfig(mode=_lib.MODE_MESH, ipd_m=0.065, max_depth=100.0)
                ctx_.call("mdvt_set_config", C.byref(cfg))
            got = res[e.name] = {}
            for label, wrong in e.all_cases():
                keep = []
                rc = fn(*arguments(e, wrong, base, at, ctx_.handle, fixture, keep))
                if e.returns == "text":
                    got[label] = [0, ""] if rc is None else [1, rc.decode()]
                elif e.returns == "value" or "ctx" not in e.by_name:
                    got[label] = [int(rc), ""]
                else:
                    got[label] = [int(rc), (L.mdvt_last_error(ctx_.handle) or b"").decode() if rc != 0 else ""]
            torch.cuda.synchronize()
            buf.copy_(pristine)                  # (an accepted call wrote its outputs: the next entry point starts from the same bytes)
            assert got["valid"][0] == 0 or e.returns == "value", f"{e.name}: the valid call was refused: {got['valid']}"
    finally:
        ctx_.close()
    return res


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="status and text of every wrong call of the table")
    ap.add_argument("--record", nargs="?", const=GOLDEN, default=None, metavar="FILE", help=f"run the cases on the GPU and write them (default {GOLDEN})")
    out = ap.parse_args().record
    if out:
        res = run_all()
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=False)
            f.write("\n")
        print(f"{out}: {sum(len(v) for v in res.values())} cases of {len(res)} entry points")
    else:
        print(__doc__)
