"""CPU: the homography RANSAC's C-ABI surface, its CPU restatement (tests/h_ref.c) against the
oracle's shared pieces and against f64 ground truth, and the two-view classification on the seeded
cases of tests/two_view_cases.py.  No GPU: the kernels are checked against h_ref bit for bit in
test_gpu_ransac_h.py."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import geometric_verification as gv
import h_ref
import oracle as O
import sfmcore
import two_view_cases as tv

IMG_AREA = tv.W * tv.H


def test_entry_points_exported_and_validate():
    lib = sfmcore.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", sfmcore.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    for name in ("sfm_ransac_h_batch", "sfm_ransac_h_counts"):
        assert name in sfmcore.EXPORTED
        assert re.search(rf"\bT {name}\b", out), name
    assert lib.sfm_version() == 5
    rp = sfmcore.RansacParams(4096, 15, 4.0, 0, 42)
    assert lib.sfm_ransac_h_batch(None, None, 0, 0, None, 1, None, None, C.byref(rp), None, None,
                                  None, None, None) == -1
    assert lib.sfm_last_error().startswith(b"sfm_ransac_h_batch")
    assert lib.sfm_ransac_h_counts(None, None, 0, 0, None, 1, None, None, C.byref(rp), None,
                                   None, None) == -1
    assert lib.sfm_last_error().startswith(b"sfm_ransac_h_counts")


def test_philox_equals_oracle():
    for ctr, key in [((0, 0, 0, 0), (0, 0)), ((1, 2, 3, 4), (42, 0)),
                     ((0xFFFFFFFF, 2, 7, 9), (0xDEADBEEF, 0x12345678)),
                     ((255, 2, 0, 1), (42, 0)), ((65535, 2, 1224, 49), (7, 1))]:
        np.testing.assert_array_equal(h_ref.philox(ctr, key), O.philox(ctr, key))


@pytest.mark.parametrize("M", [4, 5, 7, 400])
def test_sample4_distinct_in_range(M):
    for h in range(256):
        idx = h_ref.sample4(42, 3, 5, h, M)
        assert len(set(idx.tolist())) == 4, (h, idx)
        assert idx.min() >= 0 and idx.max() < M, (h, idx)


def test_sample4_uses_stream_2():
    # t = umulhi(r[k], jmax + 1) on the Philox block with counter (h, 2, a, b), key = seed
    M, seed, pa, pb, h = 400, (9 << 32) | 42, 3, 5, 17
    r = O.philox((h, 2, pa, pb), (seed & 0xFFFFFFFF, seed >> 32))
    want = []
    for k in range(4):
        jmax = M - 4 + k
        t = (int(r[k]) * (jmax + 1)) >> 32
        want.append(jmax if t in want else t)
    assert h_ref.sample4(seed, pa, pb, h, M).tolist() == want


@pytest.mark.parametrize("M", [4, 7, 64, 65, 400])
def test_normalize_equals_oracle(M):
    xy = tv.make("plane", seed=1)["kp2"][:M]
    a, b = h_ref.normalize(xy), O.normalize(xy)
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array(a[1:], np.float32).tobytes() == np.array(b[1:], np.float32).tobytes()


def _unit(Hm):
    Hm = Hm / np.linalg.norm(Hm)
    return -Hm if Hm[2, 2] < 0 else Hm


def _min_triangle_area(pts):
    areas = []
    for skip in range(4):
        a, b, c = [pts[i] for i in range(4) if i != skip]
        areas.append(0.5 * abs((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])))
    return min(areas)


def test_fit_recovers_the_plane_homography():
    """Noise-free, outlier-free plane: every valid hypothesis is the true homography.  Bound 1e-3
    in Frobenius norm a priori: f32 roundoff 6e-8 times a conditioning of at most 1e3 for samples
    whose smallest triangle covers over 1 % of the image (worse-conditioned samples are skipped)."""
    c = tv.make("plane", seed=0, noise=0.0, outlier_frac=0.0)
    Ht = _unit(tv.true_homography("plane"))
    nh = 1024  # about 6 % of the samples pass the area filter
    r = h_ref.ransac_h(c["kp1"], c["kp2"], H=nh, seed=42, pa=0, pb=1, thr=4.0, per_hyp=True)
    checked, worst = 0, 0.0
    for h in range(nh):
        if r["counts"][h] < 0:
            continue
        idx = h_ref.sample4(42, 0, 1, h, len(c["kp1"]))
        if _min_triangle_area(c["kp1"][idx].astype(np.float64)) <= 0.01 * IMG_AREA:
            continue
        Hp = gv.denormalize_H(r["hyp_H"][h], r["norm"])
        err = np.linalg.norm(Hp - Ht)
        assert err <= 1e-3, (h, err)
        checked, worst = checked + 1, max(worst, err)
    print(f"checked {checked} hypotheses, worst error {worst:.2e}")
    assert checked >= 20, checked  # the filter must leave something to check
    # every valid hypothesis explains every match of the noise-free plane
    assert r["count"] == len(c["kp1"])


def _f64_decision(Hp, kp1, kp2, sample_idx, thr):
    """Pixel-space f64 transfer decision of Hp: (inlier [M] bool, d2 [M])."""
    x1 = np.concatenate([kp1.astype(np.float64), np.ones((len(kp1), 1))], axis=1)
    q = x1 @ Hp.T
    sgn = np.sign(q[sample_idx, 2])
    assert abs(sgn.sum()) == 4, "the winner's sample lies on one side"
    with np.errstate(divide="ignore", invalid="ignore"):
        d = q[:, :2] / q[:, 2:3] - kp2.astype(np.float64)
    d2 = (d * d).sum(1)
    return (np.sign(q[:, 2]) == sgn[0]) & (d2 < thr), d2


@pytest.mark.parametrize("kind", ["plane", "rot"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_winner_decisions_against_f64(kind, seed):
    c = tv.make(kind, seed=seed)
    M, thr = len(c["kp1"]), 4.0
    r = h_ref.ransac_h(c["kp1"], c["kp2"], H=512, seed=42, pa=0, pb=1, thr=thr)
    idx = h_ref.sample4(42, 0, 1, r["best_h"], M)
    want, d2 = _f64_decision(gv.denormalize_H(r["H"], r["norm"]), c["kp1"], c["kp2"], idx, thr)
    band = np.abs(d2 - thr) <= 1e-3 * thr
    assert band.sum() <= 0.01 * M
    np.testing.assert_array_equal(r["mask"].astype(bool)[~band], want[~band])
    assert r["count"] == int(r["mask"].sum())
    planted = M - c["n_out"]
    assert planted == 280
    print(f"{kind} seed {seed}: count {r['count']} of {planted} planted, band {int(band.sum())}")
    assert r["count"] >= 0.85 * planted
    assert not r["mask"][:c["n_out"]].any(), "a planted outlier is in the mask"


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("kind", tv.KINDS)
def test_classification(kind, seed):
    c = tv.make(kind, seed=seed)
    f = O.ransac_f(c["kp1"], c["kp2"], H=1024, seed=42, pa=0, pb=1, thr=1.0)
    h = h_ref.ransac_h(c["kp1"], c["kp2"], H=512, seed=42, pa=0, pb=1, thr=4.0)
    ratio = h["count"] / f["count"]
    print(f"{kind} seed {seed}: F {f['count']} H {h['count']} ratio {ratio:.3f}")
    cls = gv.classify_two_view(f["count"], h["count"])
    if kind == "general":
        assert ratio < 0.25 and cls == "general"
    else:
        assert ratio > 0.8 and cls == "planar_or_panoramic"


def test_classify_two_view_edges():
    assert gv.classify_two_view(14, 14) == "unverified"
    assert gv.classify_two_view(0, 0) == "unverified"
    assert gv.classify_two_view(-1, -1) == "unverified"
    assert gv.classify_two_view(15, 15) == "planar_or_panoramic"
    assert gv.classify_two_view(100, 80) == "general"            # ratio must exceed 0.8
    assert gv.classify_two_view(100, 81) == "planar_or_panoramic"
    assert gv.classify_two_view(15, 14) == "general"              # H itself below min_inliers
    assert gv.classify_two_view(100, -1) == "general"
    assert gv.classify_two_view(100, 60, max_h_ratio=0.5) == "planar_or_panoramic"
    assert gv.classify_two_view(20, 20, min_inliers=30) == "unverified"
    assert gv.DEFAULT_H_THRESHOLD == 4.0 and gv.DEFAULT_MAX_H_RATIO == 0.8


def test_denormalize_H_round_trip():
    rng = np.random.default_rng(3)
    Hp = _unit(tv.true_homography("plane"))
    norm = np.array([900.0, 500.0, 0.004, 1010.0, 560.0, 0.0035])
    T1 = np.array([[norm[2], 0, -norm[2] * norm[0]], [0, norm[2], -norm[2] * norm[1]], [0, 0, 1]])
    T2 = np.array([[norm[5], 0, -norm[5] * norm[3]], [0, norm[5], -norm[5] * norm[4]], [0, 0, 1]])
    Hn = T2 @ Hp @ np.linalg.inv(T1)
    for scale in (1.0, -3.5):  # any scale and sign of the normalised H gives the same pixel H
        got = gv.denormalize_H(scale * Hn, norm)
        assert abs(np.linalg.norm(got) - 1.0) < 1e-12 and got[2, 2] >= 0
        np.testing.assert_allclose(got, Hp, atol=1e-9)
    # a pair below 4 matches reports a zero H and a zero norm: the pixel H is zero, not an error
    assert not gv.denormalize_H(np.zeros(9), np.zeros(6)).any()
    # it maps pixels like the original
    x = np.array([rng.uniform(0, tv.W), rng.uniform(0, tv.H), 1.0])
    a, b = got @ x, Hp @ x
    np.testing.assert_allclose(a[:2] / a[2], b[:2] / b[2], atol=1e-6)
