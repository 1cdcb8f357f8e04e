"""GPU: sfm_triangulate_robust equals tests/tri_ref.c byte for byte (points, mask, info, stats 0 / 2
/ 3; stats 1, the one acos, to 1e-9 degrees) on the planted-outlier, edge and batch-invariance
cases of tests/tri_cases.py; sfm_triangulate is unchanged; the incremental driver's
triangulation="ransac" option against the default on the arc scene."""
import numpy as np
import pytest

import recon
import reconstruction as R
import synth
import tri_cases
import tri_ref

pytestmark = pytest.mark.gpu


def _T(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _gpu(prob, **kw):
    ctx = R.sfmcore.context(0)
    cams, pp = _T(prob["cams"], np.float64), _T(prob["pp"], np.float64)
    out = ctx.triangulate_robust(cams, pp, _T(prob["pt_ptr"], np.int32),
                                 _T(prob["cam_idx"], np.int32),
                                 _T(prob["uv"], np.float64).reshape(-1, 2),
                                 _T(prob["pt_id"], np.int32), **kw)
    tab = ctx.triangulate_cam_table(cams, pp)
    return tuple(t.cpu().numpy() for t in out), tab.cpu().numpy()


def _same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), what


def _check(prob, name, **kw):
    (pts, stats, mask, info), tab = _gpu(prob, **kw)
    # the spec starts from the camera table: the library's own (its sincos is not libm's)
    np.testing.assert_allclose(tab, tri_ref.cam_table(prob["cams"], prob["pp"]), rtol=0,
                               atol=1e-11)
    rp, rs, rm, ri = tri_ref.run(tab, prob["pt_ptr"], prob["cam_idx"], prob["uv"], prob["pt_id"],
                                 **kw)
    _same_bytes(pts, rp, name + ": pts")
    _same_bytes(mask, rm, name + ": mask")
    _same_bytes(info, ri, name + ": info")
    _same_bytes(stats[:, [0, 2, 3]], rs[:, [0, 2, 3]], name + ": stats 0, 2, 3")
    np.testing.assert_allclose(stats[:, 1], rs[:, 1], rtol=0, atol=1e-9, err_msg=name)
    return pts, stats, mask, info


@pytest.fixture(scope="module")
def planted():
    return tri_cases.planted_outliers()


def test_planted_outliers_equal_the_reference(planted):
    pts, stats, mask, info = _check(planted, "planted")
    np.testing.assert_array_equal(mask, planted["planted"])
    assert np.linalg.norm(pts - planted["pts"], axis=1).max() < 0.25


def test_edges_equal_the_reference():
    seen = set()
    for name, prob, kw in tri_cases.edge_cases():
        pts, stats, mask, info = _check(prob, name, **kw)
        seen.update(stats[:, 3].tolist())
    assert seen == {0.0, 1.0, 4.0}


def test_batch_invariance(planted):
    base = _check(planted, "planted")
    n = len(planted["pt_id"])
    rng = np.random.Generator(np.random.PCG64(5))
    orders = [np.arange(n)[::-1], rng.permutation(n), np.arange(0, n // 3),
              np.arange(n // 3, n)]
    for i, order in enumerate(orders):
        sub = tri_cases.reorder(planted, order)
        pts, stats, mask, info = _check(sub, f"order {i}")
        _same_bytes(pts, base[0][order], f"order {i}: pts")
        _same_bytes(stats, base[1][order], f"order {i}: stats")
        _same_bytes(info, base[3][order], f"order {i}: info")
        _same_bytes(mask, base[2][sub["obs"]], f"order {i}: mask")


def test_plain_triangulate_is_unchanged(planted):
    """sfm_triangulate shares its helpers with the robust kernel now: same results as before
    (the comparison of tests/test_gpu_recon.py), also on the planted case's inputs."""
    ctx = R.sfmcore.context(0)
    prob = synth.make_ba_problem(10, 400, obs_per_pt=4, seed=0, noise_px=0.5, perturb=0.0)
    ptr = np.r_[0, np.cumsum(np.bincount(prob["pt_idx"], minlength=400))].astype(np.int32)
    sub = tri_cases.reorder(planted, np.arange(200))
    for cams, pp, p, ci, uv in ((prob["cams"], prob["pp"], ptr, prob["cam_idx"], prob["uv"]),
                                (sub["cams"], sub["pp"], sub["pt_ptr"], sub["cam_idx"],
                                 sub["uv"])):
        g, gs = (t.cpu().numpy() for t in ctx.triangulate(
            _T(cams, np.float64), _T(pp, np.float64), _T(p, np.int32), _T(ci, np.int32),
            _T(uv, np.float64)))
        o, os_ = recon.triangulate(cams, pp, p, ci, uv)
        np.testing.assert_array_equal(gs[:, 3], os_[:, 3])
        np.testing.assert_allclose(g, o, rtol=0, atol=1e-9 * np.abs(o).max())
        np.testing.assert_allclose(gs[:, :3], os_[:, :3], rtol=1e-8, atol=1e-9)


def _model(rec, scene):
    tptr, timg, tkp = rec.tracks
    obs_track = np.repeat(np.arange(len(tptr) - 1), np.diff(tptr))
    use = rec.has_point[obs_track] & rec.registered[timg]
    n_used = int((use & rec.obs_ok).sum()) if rec.obs_ok is not None else int(use.sum())
    pts_ids, pt_idx = np.unique(obs_track[use], return_inverse=True)
    err = R.reprojection_errors(rec.cams, scene["pp"], rec.points[pts_ids], timg[use],
                                pt_idx.astype(np.int32), scene["kps"][timg[use], tkp[use]])
    c_est, c_true = synth.camera_centres(rec.cams), synth.camera_centres(scene["cams"])
    s, Rm, t = synth.similarity_align(c_est, c_true)
    aligned = (s * (Rm @ c_est.T)).T + t
    return dict(points=int(rec.has_point.sum()), obs=n_used, median=float(np.median(err)),
                centre=float(np.abs(aligned - c_true).max()))


def test_driver_ransac_against_dlt():
    """The 30 x 1024 arc scene (every camera sees the whole cloud: long tracks, a quarter of the
    keypoints misplaced).  Measured on an MI355X: see DESIGN.md 4.9."""
    import incremental
    scene = synth.make_scene(30, 1024, seed=21, k1_range=0.02)
    intr = np.c_[scene["cams"][:, 6:8], scene["pp"]]
    res = {}
    for mode in ("dlt", "ransac"):
        rec = incremental.reconstruct(scene["desc"], scene["kps"], scene["n_kp"], intr,
                                      triangulation=mode)
        res[mode] = (rec, _model(rec, scene))
        print(mode, res[mode][1], "registered", int(rec.registered.sum()))
    (rd, md), (rr, mr) = res["dlt"], res["ransac"]
    assert rd.obs_ok is None
    assert np.all(rr.registered[rd.registered])
    assert mr["median"] < 0.8                          # px; keypoint noise sigma 0.5 px
    assert mr["centre"] < 0.02 * 8.0                   # 2 % of the ring radius
    assert mr["points"] >= md["points"]
    assert rr.obs_ok.dtype == bool and not rr.obs_ok.all()
