"""GPU: sfm_triangulate_multi equals tests/tri_multi_ref.py (a host loop of tri_ref.run over the
compacted remainder) byte for byte: points, info, n_points, labels, stats 0 / 2 / 3; stats 1, the
one acos, to 1e-9 degrees.  Slot 0 equals sfm_triangulate_robust of the same call.  Planted merged
tracks are recovered across every list boundary; batches are invariant; the incremental driver's
triangulation="ransac_split" option splits tracks that a wrong match merged."""
import numpy as np
import pytest

import reconstruction as R
import synth
import tri_cases
import tri_multi_cases
import tri_multi_ref
from test_gpu_triangulate_robust import _T, _model, _same_bytes
from test_triangulate_multi_cpu import check_layout, check_recovered

pytestmark = pytest.mark.gpu


def _args(prob):
    cams, pp = _T(prob["cams"], np.float64), _T(prob["pp"], np.float64)
    return (cams, pp, _T(prob["pt_ptr"], np.int32), _T(prob["cam_idx"], np.int32),
            _T(prob["uv"], np.float64).reshape(-1, 2), _T(prob["pt_id"], np.int32))


def _check(prob, name, robust=False, **kw):
    """The multi call on prob against the reference from the library's own camera table; with
    `robust` also slot 0 against Context.triangulate_robust.  Returns the GPU outputs."""
    ctx = R.sfmcore.context(0)
    args = _args(prob)
    out = tuple(t.cpu().numpy() for t in ctx.triangulate_multi(*args, **kw))
    tab = ctx.triangulate_cam_table(args[0], args[1]).cpu().numpy()
    ref = tri_multi_ref.host_loop(tab, prob, **kw)
    pts, stats, info, n_points, label = out
    rp, rs, ri, rn, rl = ref
    _same_bytes(pts, rp, name + ": pts")
    _same_bytes(info, ri, name + ": info")
    _same_bytes(n_points, rn, name + ": n_points")
    _same_bytes(label, rl, name + ": label")
    _same_bytes(stats[:, :, [0, 2, 3]], rs[:, :, [0, 2, 3]], name + ": stats 0, 2, 3")
    np.testing.assert_allclose(stats[:, :, 1], rs[:, :, 1], rtol=0, atol=1e-9, err_msg=name)
    check_layout(out, kw.get("max_points", 3), name)
    if robust:
        rkw = {k: v for k, v in kw.items() if k not in ("max_points", "min_views")}
        p1, s1, m1, i1 = (t.cpu().numpy() for t in ctx.triangulate_robust(*args, **rkw))
        _same_bytes(pts[:, 0], p1, name + ": slot 0 pts")
        _same_bytes(stats[:, 0], s1, name + ": slot 0 stats")
        _same_bytes(info[:, 0], i1, name + ": slot 0 info")
        _same_bytes((label == 0).astype(np.uint8), m1, name + ": label 0 / mask")
    return out


@pytest.fixture(scope="module")
def planted():
    return tri_cases.planted_outliers()


@pytest.fixture(scope="module")
def merges():
    return tri_multi_cases.merges()


@pytest.mark.parametrize("max_points", [1, 2, 4])
def test_equal_the_reference_and_the_single_call(planted, max_points):
    later = 0
    out = _check(planted, f"planted R={max_points}", robust=True, max_points=max_points)
    later += int((out[3] > 1).sum())
    for name, prob, kw in tri_cases.edge_cases():
        out = _check(prob, f"{name} R={max_points}", robust=True, max_points=max_points, **kw)
        later += int((out[3] > 1).sum())
    assert (later > 0) == (max_points > 1)   # outliers that agree by chance: rounds >= 1 do run


def test_planted_merges_equal_the_reference_and_are_recovered(merges):
    ends = set()
    for name, prob, kw in merges:
        out = _check(prob, name, robust=True, **kw)
        check_recovered(prob, out, name)
        stats, n_points = out[1], out[3]
        ends.update(stats[t, k, 3] for t, k in enumerate(n_points) if k < kw["max_points"])
    assert ends == {1.0, 4.0, 5.0}


def test_no_later_round():
    prob = tri_multi_cases.no_later_round()
    pts, stats, info, n_points, label = _check(prob, "no later round", robust=True, max_points=3)
    assert not n_points.any() and np.all(label == -1) and not pts.any()
    assert set(stats[:, 0, 3].tolist()) == {1.0, 4.0}
    assert np.all(stats[:, 1:, 3] == 5.0) and not stats[:, :, :3].any()
    assert np.all(info == [0, -1])


def test_batch_invariance(planted, merges):
    rng = np.random.Generator(np.random.PCG64(6))
    for what, prob in (("planted", tri_cases.reorder(planted, np.arange(600))),
                       ("merges", merges[0][1]), ("n_pt_257", merges[-1][1])):
        base = _check(prob, what, max_points=3)
        n = len(prob["pt_id"])
        orders = [np.arange(n)[::-1], rng.permutation(n), np.arange(0, n // 3),
                  np.arange(n // 3, n)]
        for i, order in enumerate(orders):
            sub = tri_cases.reorder(prob, order)
            out = _check(sub, f"{what} order {i}", max_points=3)
            for k in range(4):
                _same_bytes(out[k], base[k][order], f"{what} order {i}: output {k}")
            _same_bytes(out[4], base[4][sub["obs"]], f"{what} order {i}: label")


def test_argument_checks():
    ctx = R.sfmcore.context(0)
    args = _args(tri_multi_cases.merges()[5][1])
    for kw in (dict(max_points=0), dict(max_points=9), dict(min_views=1), dict(max_hyp=0)):
        with pytest.raises(R.sfmcore.SfmCoreError):
            ctx.triangulate_multi(*args, **kw)


# ---- the driver

def _plant_merges(scene, want=10):
    """Merges planted in the 12-image arc scene: for a point A seen in image 5, in >= 3 of the
    images 0 .. 4 and in >= 4 of 6 .. 11, its keypoint in the images 6 .. 11 is moved to the
    projection of B = C5 + 0.8 (A - C5); the descriptor stays.  B lies on A's ray from camera 5,
    so every match (5, j >= 6) survives F verification and merges the two tracks.  Returns the
    list of (A, B)."""
    ids, kps, cams, pp = scene["point_ids"], scene["kps"], scene["cams"], scene["pp"]
    C5 = synth.camera_centres(cams)[5]
    pairs = []
    for a in np.unique(ids[5][ids[5] >= 0]):
        seen = [np.nonzero(ids[i] == a)[0] for i in range(12)]
        if any(len(s) > 1 for s in seen):
            continue
        if sum(len(s) for s in seen[:5]) < 3 or sum(len(s) for s in seen[6:]) < 4:
            continue
        A = scene["pts"][a]
        B = C5 + 0.8 * (A - C5)
        new = {}
        for j in range(6, 12):
            if len(seen[j]):
                Rj = synth.angle_axis_to_rotmat(cams[j, :3])
                uv, z = synth.project(Rj, cams[j, 3:6], cams[j, 6], cams[j, 7], pp[j, 0], pp[j, 1],
                                      B[None])
                assert z[0] > 0 and 0 <= uv[0, 0] < synth.WIDTH and 0 <= uv[0, 1] < synth.HEIGHT
                new[j] = uv[0]
        for j, uv in new.items():
            kps[j, seen[j][0]] = uv
        assert np.linalg.norm(A - B) >= 1.2
        pairs.append((A, B))
        if len(pairs) == want:
            break
    return pairs


def _aligned_points(rec, scene):
    c_est, c_true = synth.camera_centres(rec.cams), synth.camera_centres(scene["cams"])
    reg = rec.registered
    s, Rm, t = synth.similarity_align(c_est[reg], c_true[reg])
    return (s * (Rm @ rec.points[rec.has_point].T)).T + t


def test_driver_splits_planted_merges():
    import incremental
    scene = synth.make_scene(12, 1024, seed=21, k1_range=0.02, misplace_frac=0.0)
    pairs = _plant_merges(scene)
    assert len(pairs) >= 10
    intr = np.c_[scene["cams"][:, 6:8], scene["pp"]]
    res = {}
    for mode in ("ransac", "ransac_split"):
        kw = dict(split=dict(max_points=3, min_views=2)) if mode == "ransac_split" else {}
        rec = incremental.reconstruct(scene["desc"], scene["kps"], scene["n_kp"], intr,
                                      triangulation=mode, **kw)
        res[mode] = (rec, _model(rec, scene), _aligned_points(rec, scene))
        print(mode, res[mode][1], "registered", int(rec.registered.sum()),
              "split", getattr(rec, "n_split", None))
    (rr, mr, pr), (rs, ms, ps) = res["ransac"], res["ransac_split"]
    near = lambda P, X: bool((np.linalg.norm(P - X, axis=1) < 0.1).any())
    for A, B in pairs:
        assert near(ps, A) and near(ps, B)
        assert not (near(pr, A) and near(pr, B))
    assert rs.n_split >= len(pairs) and rr.n_split == 0
    np.testing.assert_array_equal(rs.registered, rr.registered)
    for m in (mr, ms):
        assert m["median"] < 0.8                          # px; keypoint noise sigma 0.5 px
        assert m["centre"] < 0.02 * 8.0                   # 2 % of the ring radius
    # the tracks stay track-major and contiguous, and every split track has its point
    tptr, timg, tkp = rs.tracks
    assert len(tptr) - 1 == len(rs.has_point) == len(rs.points)
    assert tptr[-1] == len(timg) == len(rs.obs_ok) and np.all(np.diff(tptr) >= 0)
    otr = rs.obs_d[0].cpu().numpy()
    np.testing.assert_array_equal(otr, np.repeat(np.arange(len(tptr) - 1), np.diff(tptr)))


def test_driver_split_does_not_regress_the_arc_scene():
    import incremental
    scene = synth.make_scene(30, 1024, seed=21, k1_range=0.02)
    intr = np.c_[scene["cams"][:, 6:8], scene["pp"]]
    res = {}
    for mode in ("ransac", "ransac_split"):
        rec = incremental.reconstruct(scene["desc"], scene["kps"], scene["n_kp"], intr,
                                      triangulation=mode)
        res[mode] = (rec, _model(rec, scene))
        print(mode, res[mode][1], "registered", int(rec.registered.sum()))
    (rr, mr), (rs, ms) = res["ransac"], res["ransac_split"]
    np.testing.assert_array_equal(rs.registered, rr.registered)
    assert ms["points"] >= mr["points"]
    assert ms["median"] < 0.8 and ms["centre"] < 0.02 * 8.0


def test_driver_names_the_three_values():
    import incremental
    with pytest.raises(ValueError, match="'dlt', 'ransac' or 'ransac_split'"):
        incremental.reconstruct(None, None, None, None, triangulation="split")
