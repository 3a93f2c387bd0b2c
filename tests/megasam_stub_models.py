"""A stub in the camera tracker's place for the MegaSAM step's tests and tools (tools/sam_track_video.py --generator
megasam_stub_models:make_tracker, with tests/ on the path): the tracker's contract of INTEGRATION.md on CUDA tensors, around a
deterministic NumPy heart (core) that tests/megasam_ref.run_step calls on its own model inputs.  The poses are a function of the frame
number, the depth and the motion map functions of the planes the tracker was handed at an eighth of their size (so a frame that
reached the tracker changed shows up in the files).  The stub records what it was handed and checks shapes, types and devices.
Plain module: no fixture, no pytest setting."""
import numpy as np

F = np.float32
TRACKERS = []                                                       # every tracker make_tracker made, in order


def core(items):
    """items: [(t, image uint8 [1, 3, h, w], depth float32 [h, w], intrinsics float32 [4], mask float32 [h, w])] as NumPy arrays ->
    (traj float32 [t, 7], depth_est float32 [t, h / 8, w / 8], motion_prob float32 [t, h / 8, w / 8], intrinsics float32 [t, 4])."""
    traj, depths, motions, intr = [], [], [], []
    for i, image, depth, k, mask in items:
        a = 0.02 * i
        traj.append([0.01 * i, -0.02 * i, 0.005 * i * i, 0.0, np.sin(a / 2), 0.0, np.cos(a / 2)])        # a turn about y that grows
        green = image[0, 1, 4::8, 4::8].astype(F) / F(255)
        red = image[0, 0, 4::8, 4::8].astype(F) / F(255)
        depths.append(depth[4::8, 4::8] * F(1.25) + green - F(0.5))                 # below 0 and beyond max_depth in places
        motions.append(mask[4::8, 4::8] * F(1.3) - F(0.15) + red * F(0.2))          # below 0 and above 1 in places
        intr.append(np.asarray(k, F) / F(8))
    return np.array(traj, F), np.stack(depths).astype(F), np.stack(motions).astype(F), np.stack(intr).astype(F)


class StubTracker:
    def __init__(self, image_size):
        self.image_size = [int(v) for v in image_size]
        self.handed, self.final, self.optimize_intrinsic = [], None, None

    def _take(self, t, image, depth, intrinsics, mask):
        import torch
        h, w = self.image_size
        assert t == len(self.handed), "the frames come in order"
        assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in (image, depth, intrinsics, mask))
        assert image.dtype == torch.uint8 and image.shape == (1, 3, h, w)
        assert depth.dtype == torch.float32 and depth.shape == (h, w) and mask.dtype == torch.float32 and mask.shape == (h, w)
        assert intrinsics.dtype == torch.float32 and intrinsics.shape == (4,)
        self.handed.append((t, image.cpu().numpy(), depth.cpu().numpy(), intrinsics.cpu().numpy(), mask.cpu().numpy()))

    def track(self, t, image, depth, intrinsics, mask):
        assert self.final is None, "track_final is the last call"
        self._take(t, image, depth, intrinsics, mask)

    def track_final(self, t, image, depth, intrinsics, mask):
        assert self.final is None
        self._take(t, image, depth, intrinsics, mask)
        self.final = t

    def terminate(self, stream, optimize_intrinsic):
        import torch
        stream = list(stream)
        assert [s[0] for s in stream] == [s[0] for s in self.handed]
        for s, kept in zip(stream, self.handed):                    # the stream holds what was handed over, frame by frame
            assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(s[1:], kept[1:]))
        self.optimize_intrinsic = optimize_intrinsic
        dev = stream[0][1].device
        return tuple(torch.from_numpy(v).to(dev) for v in core(self.handed))


def make_tracker(image_size):
    TRACKERS.append(StubTracker(image_size))
    return TRACKERS[-1]
