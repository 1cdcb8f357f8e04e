"""CPU: the host-side pieces of reconstruct(triangulation="ransac_split") on CPU tensors: the
rebuild that moves observations to new tracks keeps every array track-major and contiguous, and
the driver's device reprojection agrees with synth.project."""
import numpy as np
import pytest
import torch

import incremental
import synth


def _rec(lens, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    n_tr, n_obs = len(lens), int(sum(lens))
    ptr = torch.from_numpy(np.r_[0, np.cumsum(lens)].astype(np.int32))
    img = torch.from_numpy(rng.integers(0, 9, n_obs).astype(np.int32))
    kp = torch.arange(n_obs, dtype=torch.int32)           # unique: identifies an observation
    kps = torch.from_numpy(rng.uniform(0, 100, size=(9, n_obs, 2)))
    rec = incremental.Reconstruction(9)
    rec._tracks_d = (ptr, img, kp)
    rec.obs_d = incremental.track_observations(ptr, img, kp, kps)
    rec.obs_ok_d = torch.from_numpy(rng.random(n_obs) < 0.8)
    rec.pts_d = torch.from_numpy(rng.normal(size=(n_tr, 3)))
    rec.has_d = torch.from_numpy(rng.random(n_tr) < 0.5)
    return rec, kps


def test_move_observations_keeps_the_arrays_track_major():
    lens = [3, 0, 5, 2, 7, 1]
    rec, kps = _rec(lens)
    before = dict(zip(rec._tracks_d[2].tolist(),
                      zip(rec.obs_d[0].tolist(), rec.obs_d[1].tolist(), rec.obs_ok_d.tolist())))
    old_pts, old_has = rec.pts_d.clone(), rec.has_d.clone()
    # track 2 gives its 2nd and 4th observation to track 6, track 4 three to 7 and two to 8
    obs = torch.tensor([4, 6, 10, 11, 13, 14, 16])
    track = torch.tensor([6, 6, 7, 8, 7, 7, 8])
    new_pts = torch.arange(9, dtype=torch.float64).reshape(3, 3)
    moved = dict(zip(rec._tracks_d[2][obs].tolist(), track.tolist()))
    incremental._move_observations(rec, obs, track, new_pts)
    otr, timg, oxy = rec.obs_d
    ptr, img, kp = (t.numpy() for t in rec._tracks_d)
    assert rec.tracks[0] is not None and len(ptr) == 10 and ptr[-1] == sum(lens)
    np.testing.assert_array_equal(np.diff(ptr), [3, 0, 3, 2, 2, 1, 2, 3, 2])
    np.testing.assert_array_equal(otr.numpy(), np.repeat(np.arange(9), np.diff(ptr)))
    np.testing.assert_array_equal(img, timg.numpy())
    for i, k in enumerate(kp.tolist()):
        tr, im, ok = before[k]
        assert otr[i] == moved.get(k, tr) and timg[i] == im and rec.obs_ok_d[i] == ok
        np.testing.assert_array_equal(oxy[i].numpy(), kps[im, k].numpy())
    for t in range(9):     # the order inside a track is the old one
        assert np.all(np.diff(kp[ptr[t]:ptr[t + 1]]) > 0)
    assert torch.equal(rec.pts_d[:6], old_pts) and torch.equal(rec.pts_d[6:], new_pts)
    assert torch.equal(rec.has_d[:6], old_has) and bool(rec.has_d[6:].all())
    assert rec.points.shape == (9, 3) and rec.has_point.shape == (9,)


def test_reprojection_equals_synth_project():
    rng = np.random.Generator(np.random.PCG64(1))
    scene = synth.make_scene(4, 64, seed=3, k1_range=0.02)
    cams = scene["cams"].copy()
    cams[0, :3] = 0.0                                     # the zero rotation's branch
    X = rng.uniform(-2, 2, size=(40, 3))
    img = rng.integers(0, 4, 40)
    xy = rng.uniform(0, 1000, size=(40, 2))
    err, depth = incremental._reprojection(torch.from_numpy(cams), torch.from_numpy(scene["pp"]),
                                           torch.from_numpy(X), torch.from_numpy(img),
                                           torch.from_numpy(xy))
    for i in range(40):
        c = cams[img[i]]
        uv, z = synth.project(synth.angle_axis_to_rotmat(c[:3]), c[3:6], c[6], c[7],
                              *scene["pp"][img[i]], X[i][None])
        assert abs(float(depth[i]) - z[0]) < 1e-12
        assert abs(float(err[i]) - np.linalg.norm(uv[0] - xy[i])) < 1e-9


def test_the_error_names_three_values():
    with pytest.raises(ValueError, match="'dlt', 'ransac' or 'ransac_split'"):
        incremental.reconstruct(None, None, None, None, triangulation="split")
