"""Expected values for the two entry points of include/mdvt_infill_engines.h and for the clip schedules of
metric_depth_video_toolbox_amd/m2svid_infill.py and stereo_dissoclusion_net_infill.py, run on the test machine.

The m2svid inputs and chunks are composed from tests/infill_adapter_ref.py (resize_u8, eye_of, composite_eye: the NumPy restatement
of include/mdvt_infill_adapter.h).  The finish is composed, in Python, from the plain-C oracle's own functions -- box_blur4,
mark_lower_side, dilate_cross, blur_under_mask (oracle/c_oracle.py) -- the very functions orc_normal_infill is made of, which
tests/golden/normal_infill.npz holds to the reference's basic_nomal_infill.normal_infill."""
import numpy as np

import infill_adapter_ref as R

FRAMES_CHUNK = R.FRAMES_CHUNK
BLUE = np.array([0, 0, 255], dtype=np.uint8)


# ---- m2svid -------------------------------------------------------------------------------------------------------------------

def m2s_prepare_eye(sbs_color, sbs_mask, org, eye, image_size, mask_size):
    """m2s:224-261 -> (image [N,ih,iw,3], org_image [N,ih,iw,3], mask [N,mh,mw], hole counts [N])."""
    (iw, ih), (mw, mh) = image_size, mask_size
    images, orgs, masks = [], [], []
    for c, m, o in zip(sbs_color, sbs_mask, org):
        c, m = R.eye_of(c, eye), R.eye_of(m, eye)
        if eye == 0:
            c, m, o = c[:, ::-1], m[:, ::-1], o[:, ::-1]
        plane = (m != 0).any(axis=-1).astype(np.uint8) * 255
        images.append(R.resize_u8(np.ascontiguousarray(c), iw, ih))
        orgs.append(R.resize_u8(np.ascontiguousarray(o), iw, ih))
        masks.append(((R.resize_u8(np.ascontiguousarray(plane), mw, mh) > 0) * 255).astype(np.uint8))
    masks = np.array(masks)
    return np.array(images), np.array(orgs), masks, (masks.reshape(len(masks), -1) == 255).sum(axis=1).astype(np.uint32)


def m2s_deal_with_frame_chunk(first, color, mask, org, last, fps, generate, orc, image_size, mask_size):
    """One chunk on the host (m2s:211-332).  generate(frames, masks, org_frames, fps) -> frames on NumPy arrays.  -> (start, pasted,
    blended) of the written frames."""
    T = len(color)
    start, end = (0 if first else 3), (T if last else T - 3)
    halves = []
    for eye in (0, 1):
        image, org_image, mmask, counts = m2s_prepare_eye(color, mask, org, eye, image_size, mask_size)
        frames = image if counts.sum() == 0 else generate(image, mmask, org_image, fps)          # (no colour match: m2s:275, 284)
        halves.append(R.composite_eye(frames[start:end], color[start:end], mask[start:end], eye, orc))
    if end <= start:
        empty = np.empty((0,) + color.shape[1:], dtype=np.uint8)
        return start, empty, empty
    return start, np.concatenate([halves[0][0], halves[1][0]], axis=2), np.concatenate([halves[0][1], halves[1][1]], axis=2)


def m2s_run_clip(color, mask, org, fps, generate, orc, blend, image_size, mask_size):
    """The whole schedule (m2s:398-453) on host arrays: color [N,H,2W,3], mask [M,H,2W,3] (M < N: black masks for the rest), org
    [>= N,oh,ow,3] -> (output frames [N,H,2W,3]: blended with `blend`, else pasted; [(first, last, buffered frames)] per call).  The
    kept pasted frames T-6 .. T-4 go with their own masks and original frames."""
    n = len(color)
    assert n >= 1 and len(org) >= n
    full_mask = np.zeros_like(color)
    full_mask[:min(n, len(mask))] = mask[:n]
    out, calls, buf, first = [], [], [], True
    for t in range(n):
        buf.append((color[t], full_mask[t], org[t]))
        if len(buf) >= FRAMES_CHUNK:
            c, m, o = (np.array([b[k] for b in buf]) for k in range(3))
            start, pasted, blended = m2s_deal_with_frame_chunk(first, c, m, o, False, fps, generate, orc, image_size, mask_size)
            calls.append((first, False, len(buf)))
            out.extend(blended if blend else pasted)
            T = len(buf)
            buf = [(pasted[T - 6 - start + i], m[T - 6 + i], o[T - 6 + i]) for i in range(3)] + buf[-3:]
            first = False
    c, m, o = (np.array([b[k] for b in buf]) for k in range(3))
    _, pasted, blended = m2s_deal_with_frame_chunk(first, c, m, o, True, fps, generate, orc, image_size, mask_size)
    calls.append((first, True, len(buf)))
    out.extend(blended if blend else pasted)
    return np.array(out), calls


# ---- the finish (sdn:100-123 behind the model) ----------------------------------------------------------------------------------

def finish_stages(img, model, infill_mask, orc):
    """One image [H,W,3] -> (out, dict(bg, work, marks, grown))."""
    img, model, infill_mask = (np.ascontiguousarray(a, dtype=np.uint8) for a in (img, model, infill_mask))
    bg = (infill_mask != 0).all(axis=-1)                                               # sdn:101
    work = img.copy()
    work[bg] = orc.box_blur4(model)[bg]                                                # sdn:108-111
    marks = (orc.mark_lower_side(infill_mask, 30) == BLUE).all(axis=-1)                # sdn:115-116
    grown = orc.dilate_cross(marks, 6)                                                 # sdn:119
    return orc.blur_under_mask(work, grown), dict(bg=bg, work=work, marks=marks, grown=grown)      # sdn:122


def finish(img, model, infill_mask, orc):
    """[N,H,W,3] (or one image [H,W,3]) -> the finished images."""
    if np.ndim(img) == 3:
        return finish_stages(img, model, infill_mask, orc)[0]
    return np.array([finish_stages(i, p, m, orc)[0] for i, p, m in zip(img, model, infill_mask)])


def sdn_run_clip(color, mask, depth, generate, orc):
    """sdn:165-216 on host arrays: color, depth [N,H,2W,3], mask [M,H,2W,3] (M < N: black masks for the rest).  generate(image,
    infill_mask, depth) -> image on NumPy arrays [1,H,W,3], [1,H,W,3], float32 [1,H,W]."""
    n = len(color)
    full_mask = np.zeros_like(color)
    full_mask[:min(n, len(mask))] = mask[:n]
    out = np.empty_like(color)
    for t in range(n):
        for eye in (0, 1):
            img, m, d = (np.ascontiguousarray(R.eye_of(a[t], eye)) for a in (color, full_mask, depth))
            percent = orc.decode_depth(d, 1.0)                                         # sdn:95
            model = generate(img[None], m[None], percent[None])[0]
            R.eye_of(out[t], eye)[...] = finish(img, model, m, orc)
    return out


# ---- test inputs ----------------------------------------------------------------------------------------------------------------

def finish_masks(rng, H, W, kind):
    """An infill-mask image [H,W,3] for the finish."""
    m = np.zeros((H, W, 3), dtype=np.uint8)
    if kind == "none":
        return m
    if kind == "all":                                               # every pixel a hole and bg: no channel is zero
        m[...] = rng.integers(1, 256, m.shape, dtype=np.uint8)
        return m
    if kind == "borders":                                           # holes on each border and in each corner; normals pointing into the image and out of it
        t = max(1, min(4, min(H, W) // 5))
        m[:, :t] = (1, 128, 77)                                     # left, pointing left (the march leaves the image at once)
        m[:, W - t:] = (255, 127, 1)                                # right, pointing right (likewise)
        m[:t, :] = (128, 255, 200)                                  # top, pointing down: its lower side lies within six pixels of the border
        m[H - t:, :] = (127, 1, 9)                                  # bottom, pointing up
        m[0, 0], m[0, W - 1], m[H - 1, 0], m[H - 1, W - 1] = (255, 255, 3), (1, 255, 3), (255, 1, 3), (1, 1, 3)      # corners pointing inwards
        return m
    if kind == "pixels":                                            # one-pixel holes with normals in all four quadrants and on the axes
        cols = [(255, 255, 9), (1, 255, 9), (1, 1, 9), (255, 1, 9), (255, 128, 9), (1, 128, 9), (128, 255, 9), (128, 1, 9), (127, 127, 9), (128, 128, 1)]
        for k in range(max(2, H * W // 12)):
            m[int(rng.integers(0, H)), int(rng.integers(0, W))] = cols[k % len(cols)]
        return m
    if kind == "deep":                                              # one hole deeper than the 30 steps of the lower-side march, every direction
        m[1:H - 1, 1:W - 1] = (255, 128, 50)
        m[1:H - 1, 1:(W - 1) // 2] = (1, 129, 50)
        return m
    if kind == "zero_channel":                                      # non-black mask pixels with a zero channel: they march, but are not bg
        for (ya, yb, xa, xb), c in (((1, H // 2, 1, W // 2), (0, 255, 40)), ((H // 2, H - 1, W // 2, W - 1), (255, 0, 40)),
                                    ((1, H // 2, W // 2, W - 1), (128, 255, 0)), ((H // 2, H - 1, 1, W // 2), (200, 20, 7))):
            m[ya:yb, xa:xb] = c
        return m
    if kind == "directions":                                        # eight holes a few pixels across: normals in all four quadrants and on the axes
        cols = [(255, 255, 9), (1, 255, 9), (1, 1, 9), (255, 1, 9), (255, 128, 9), (1, 128, 9), (128, 255, 9), (128, 1, 9)]
        h, w = max(1, H // 3 - 1), max(1, W // 5 - 1)
        for k, c in enumerate(cols):
            y, x = (k // 4) * (H // 2) + 1, (k % 4) * (W // 4) + 1
            m[y:min(y + h, H), x:min(x + w, W)] = c
        return m
    assert kind == "mixed"
    for _ in range(5):
        h, w = int(rng.integers(1, max(H // 2, 2))), int(rng.integers(1, max(W // 2, 2)))
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        c = rng.integers(0, 256, 3)
        if rng.random() < 0.7:
            c = np.maximum(c, 1)
        m[y:y + h, x:x + w] = c
    return m


FINISH_KINDS = ("none", "all", "borders", "pixels", "directions", "deep", "zero_channel", "mixed")
