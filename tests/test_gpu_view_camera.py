"""The camera of view_depthfile end to end on the GPU: the centres of a posed batch, read back once, become targets, the targets
views, the views the records of a posed render -- and that render's left eye is the oracle's for make_params(ipd_m = 0,
T = V @ T_frame), bit for bit, with the scene in sight.  (Here the render is the stereo call with pupillary distance 0 -- both eyes are the
view --: view_params' records are a posed render's.  tests/test_gpu_view_render.py holds the single-image call.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("pointcloud", [False, True], ids=["mesh", "points"])
def test_a_view_is_a_posed_render_aimed_at_the_centre(pointcloud):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from metric_depth_video_toolbox_amd import view_depthfile as vd
    from metric_depth_video_toolbox_amd.stereo_rerender import StereoRerenderer
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene, synthetic_pose_track
    from oracle import c_oracle as co
    import view_ref as vr

    W, H, N = 96, 64, 2
    scene = SyntheticScene(W, H, config_id=1, n_fg=4)
    frames = [scene.frame(k) for k in range(N)]
    depth, color = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    track = synthetic_pose_track(8)[[0, 7]]                          # the identity, and a pose
    r = StereoRerenderer(W, H, device=0, pupillary_distance=0, render_as_pointcloud=pointcloud)
    try:
        params = [r.frame_params(xfov=45.0, transformation=track[k]) for k in range(N)]
        assert params[0].depth_scale == 1.0                          # the viewer has no master fov
        K = np.array([params[0].K[i] for i in range(9)]).reshape(3, 3)
        d_depth, d_color = torch.from_numpy(depth).cuda(), torch.from_numpy(color).cuda()
        centres = vd.centers(d_depth, params, r).cpu().numpy()       # the one read-back of the batch
        want_c = np.stack([vr.center(depth[k], K, mesh=not pointcloud, T=track[k]) for k in range(N)])
        assert centres.tobytes() == want_c.tobytes()
        zc = float(centres[0, 2])
        cam = vd.camera_position(0.2 * zc, 0.2 * zc, -0.4 * zc)      # the default 2, 2, -4 scaled to the scene
        views = np.stack([vd.look_at_view(cam, vd.look_at_target(centres[k], ty=-99.0)) for k in range(N)])
        for k in range(N):                                           # the target is straight ahead: it projects to the image centre
            t = views[k] @ np.append(centres[k], 1.0)
            assert abs(t[0]) < 1e-12 * zc and abs(t[1]) < 1e-12 * zc and t[2] > 0
        got = r.render(d_depth, d_color, vd.view_params(params, views), want_depth=True)
        sbs, mask, z = got["sbs"].cpu().numpy(), got["mask"].cpu().numpy(), got["depth"].cpu().numpy()
        for k in range(N):
            op = co.make_params(W, H, K, ipd_m=0.0, max_depth=100.0, depth_scale=1.0, mode=co.MODE_POINTS if pointcloud else co.MODE_MESH,
                                T=views[k] @ track[k])
            want = co.render_stereo(op, depth[k], color[k], want_depth=True)
            assert np.array_equal(sbs[k, :, :W], want["left_rgb"]) and np.array_equal(mask[k, :, :W], want["left_mask"])
            assert np.array_equal(z[k, :, :W], want["left_depth"])
            assert np.array_equal(sbs[k, :, W:], sbs[k, :, :W]) and np.array_equal(mask[k, :, W:], mask[k, :, :W])      # ipd 0: one view, twice
            seen = want["left_mask"] == 0
            assert seen.mean() > (0.02 if pointcloud else 0.2), f"frame {k}: the camera does not see the scene ({seen.mean():.3f})"
            assert not np.array_equal(want["left_rgb"], color[k])    # ... and not from where the video was taken
    finally:
        r.close()
