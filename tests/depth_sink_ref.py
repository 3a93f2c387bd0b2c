"""The expected values of the depth sink's tests: save_depth_video behind the NaN rule and the batch factor as
include/mdvt_depth_sink.h states them, and the Depth-Anything-3 step around a model (tools/video_da3.py) from the schedule to the
written poses, run by NumPy on the test machine, never by the library.  Built on tests/metric_align_ref.py's resize_linear, code and
fit, which tests/golden already holds to the reference's own functions.  Plain module: no fixture, no pytest setting."""
import numpy as np

import metric_align_ref as mr

F = np.float32


# ---- the sink -------------------------------------------------------------------------------------------------------------------
def sink(x, max_depth, out_size=None, scale=None, nan_to_max=False, bgr=False):
    """metric planes [N, H, W] -> (codes uint8 [N, H', W', 3], c float32 [N, H', W']).  scale: None, or the float32 factor."""
    codes, planes = [], []
    for plane in np.asarray(x, F):
        d = plane.copy()
        with np.errstate(all="ignore"):
            if nan_to_max:
                d[np.isnan(d)] = float(max_depth)                   # moge_video.py:171
            if scale is not None:
                d *= float(F(scale))                                # vd3:193: a float32 array times a Python float, in float32
            assert d.dtype == np.float32
            if out_size is not None:
                d = mr.resize_linear(d, int(out_size[0]), int(out_size[1]))
        c, rgb = mr.code(np.where(np.isnan(d), F(0), d), max_depth, bgr)
        c = np.where(np.isnan(d), d, c)                             # a NaN has no defined code: the header gives it code 0 and keeps it in the plane
        codes.append(rgb)
        planes.append(c)
    return np.stack(codes), np.stack(planes)


def batch_scale(a, b):
    """s with a ~ s * b: float32(sum(a b) / max(sum(b b), 1e-12)), the two sums fit's b_0 and a_00 with prediction b and target a."""
    v = mr.fit(mr.concat(b), mr.concat(a))
    with np.errstate(all="ignore"):
        return F(v[3] / np.maximum(v[0], F(1e-12)))                  # (a NaN sum stays NaN)


# ---- the step ---------------------------------------------------------------------------------------------------------------------
def schedule(n, images_per_batch, batch_overlap, nr_of_ref_frames):
    """[(the frames the model sees, how many of them lead as references)] per batch, written as the plain loops of vd3:128-171."""
    refs = []
    if nr_of_ref_frames != 0:
        nth = n // nr_of_ref_frames
        if nth != 0:
            for i in range(n):
                if i % nth == 0:
                    refs.append(i)
        else:
            refs.append(0)
    batches = []
    for i in range(n):
        if i % images_per_batch == 0:
            batches.append([])
        batches[-1].append(i)
    out, last = [], None
    for batch in batches:
        ids, used = list(refs), len(refs)
        if last is not None:
            ids.extend(last)
            used = len(ids)
        ids.extend(batch)
        out.append((ids, used))
        last = batch[-batch_overlap:]
    return out


def h4(p):
    """[3, 4] -> [4, 4] in float64."""
    return np.vstack([np.asarray(p, np.float64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])


def centres(poses):
    poses = np.asarray(poses, np.float64)
    return np.stack([-p[:3, :3].T @ p[:3, 3] for p in poses])


def umeyama(src, dst):
    """(s, R, t) with dst ~ s R src + t over [n, 3] points: Umeyama's closed form; the identity where fewer than 3 points or a zero
    variance leave it undefined."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    ident = (1.0, np.eye(3), np.zeros(3))
    if len(src) < 3:
        return ident
    ms, md = src.mean(0), dst.mean(0)
    xs, xd = src - ms, dst - md
    var = (xs ** 2).sum() / len(src)
    if not np.isfinite(var) or var <= 1e-18 or not np.isfinite(xd).all():
        return ident
    cov = xd.T @ xs / len(src)
    U, D, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    s = float((D * np.diag(S)).sum() / var)
    if not np.isfinite(s) or s <= 0:
        return ident
    return s, R, md - s * R @ ms


def apply_sim3(poses, s, R, t):
    out = []
    for p in np.asarray(poses, np.float64):
        c = s * R @ (-p[:3, :3].T @ p[:3, 3]) + t
        Rn = p[:3, :3] @ R.T
        out.append(np.hstack([Rn, (-Rn @ c)[:, None]]))
    return np.stack(out) if out else np.zeros((0, 3, 4))


def run_step(frames, infer, *, max_depth, images_per_batch, batch_overlap, nr_of_ref_frames, resolution=504, out_size=None):
    """The whole step on host arrays.  frames uint8 [n, H, W, 3]; infer(frames [T, H, W, 3], resolution) -> (depth float32
    [T, h, w], extrinsics [T, 3, 4], intrinsics [T, 3, 3]) in NumPy.  -> (codes [n, H, W, 3], xfovs [n], transformations [n, 4, 4],
    the batches' factors)."""
    n, H, W = frames.shape[:3]
    ow, oh = (W, H) if out_size is None else out_size
    codes, intr_out, ext_out, factors = [], [], [], []
    align_depths = align_ext = last_depth = last_ext = None
    for ids, used in schedule(n, images_per_batch, batch_overlap, nr_of_ref_frames):
        depth, ext, intr = infer(frames[ids], resolution)
        depth, ext, intr = np.array(depth, F), np.array(ext, np.float64), np.array(intr)
        s = None
        if align_depths is None:
            align_depths = depth[:used].copy()
        if last_depth is not None:
            s = batch_scale(np.concatenate([align_depths, last_depth]), depth[:used])
            ext[:, :, 3] *= float(s)
            with np.errstate(all="ignore"):
                depth = depth * float(s)
            assert depth.dtype == np.float32
            factors.append(s)
        ref_ext = ext[:used]
        if align_ext is None:
            align_ext = ref_ext.copy()
        new_ext = ext[used:]
        if last_ext is not None:
            earlier = np.concatenate([align_ext, last_ext])
            sim = umeyama(centres(ref_ext), centres(earlier))
            new_ext, ref_ext = apply_sim3(new_ext, *sim), apply_sim3(ref_ext, *sim)
            diff = h4(earlier[-1]) @ np.linalg.inv(h4(ref_ext[-1]))
            new_ext = np.stack([(diff @ h4(v))[:3] for v in new_ext])
        codes.append(sink(depth[used:], max_depth, (ow, oh))[0])
        intr_out.extend(intr[used:])
        ext_out.extend(new_ext)
        handed = len(ids[used:][-batch_overlap:])                   # the frames the next batch sees again; their planes and poses go with them
        last_ext, last_depth = new_ext[-handed:], depth[-handed:]
    xfovs = [float(np.rad2deg(2 * np.arctan2(K[0][2] * 2, 2 * K[0][0]))) for K in intr_out]      # in the intrinsics' own dtype
    return np.concatenate(codes), xfovs, np.stack([np.linalg.inv(h4(e)) for e in ext_out]), factors
