"""CPU: the two-view pose spec itself (tests/pose_ref.c) against ground truth, numpy and the host
routine incremental.relative_pose, on the seeded cases of tests/two_view_cases.py; and the C-ABI
surface of sfm_two_view_pose_batch.  No GPU: the kernels are compared with pose_ref bit for bit in
test_gpu_two_view_pose.py."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import geometric_verification as gv
import incremental
import oracle as O
import pose_ref
import sfmcore
import two_view_cases as tv

INTR = np.array([tv.F_PX, 0.0, tv.PP[0], tv.PP[1]])
SEEDS = [0, 1, 2, 3]
_CACHE = {}


def fitted(kind, seed, mask="oracle"):
    """(case, x1, x2, mask, pose_ref result) with the inliers from O.ransac_f's mask ("oracle") or
    the case's true inliers ("true": every match that is not a planted outlier)."""
    key = (kind, seed, mask)
    if key not in _CACHE:
        c = tv.make(kind, seed)
        x1, x2 = pose_ref.undistort(c["kp1"], INTR), pose_ref.undistort(c["kp2"], INTR)
        if mask == "oracle":
            mk = O.ransac_f(c["kp1"], c["kp2"], H=4096, seed=42, pa=0, pb=1)["mask"]
        else:
            mk = (np.arange(len(x1)) >= c["n_out"])
        mk = np.ascontiguousarray(mk, np.uint8)
        _CACHE[key] = (c, x1, x2, mk, pose_ref.pose(x1, x2, mk))
    return _CACHE[key]


def truth(c):
    Rt = c["R2"] @ c["R1"].T
    return Rt, c["t2"] - Rt @ c["t1"]


def rot_angle_deg(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0)))


def vec_angle_deg(a, b):
    return np.degrees(np.arccos(np.clip(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)), -1, 1)))


def test_entry_point_exported_and_validates():
    lib = sfmcore.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", sfmcore.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert "sfm_two_view_pose_batch" in sfmcore.EXPORTED
    assert re.search(r"\bT sfm_two_view_pose_batch\b", out)
    assert lib.sfm_version() == 5   # an additive entry point
    prm = sfmcore.TwoViewPoseParams(C.sizeof(sfmcore.TwoViewPoseParams), 15, 0.001)
    outputs = [None] * 5
    assert lib.sfm_two_view_pose_batch(None, None, 0, 0, None, 1, None, None, None, None, None,
                                       C.byref(prm), *outputs) == -1
    assert lib.sfm_last_error().startswith(b"sfm_two_view_pose_batch")
    assert C.sizeof(sfmcore.TwoViewPoseParams) == 12
    assert sfmcore.TwoViewPoseParams._fields_[0][0] == "struct_size"


@pytest.mark.parametrize("seed", SEEDS)
def test_general_pose_from_the_oracle_mask(seed):
    """The issue's bounds, measured with the oracle's mask (seeds 0-3): R error 0.05-0.66 deg,
    t error 0.45-1.60 deg, every inlier in front, median angle 10.3-11.6 deg: none needed
    widening."""
    c, x1, x2, mk, r = fitted("general", seed)
    Rt, tt = truth(c)
    st = r["stat"]
    assert st[0] == 0 and st[7] == mk.sum()
    assert rot_angle_deg(r["R"].reshape(3, 3), Rt) < 1.0
    assert vec_angle_deg(r["t"], tt) < 2.0
    assert st[2 + st[1]] >= 0.95 * st[7]
    assert 9.0 < pose_ref.key_to_degrees(r["median_key"]) < 13.0
    assert gv.key_to_degrees(r["median_key"]) == float(pose_ref.key_to_degrees(r["median_key"]))


@pytest.mark.parametrize("seed", SEEDS)
def test_rot_pose(seed):
    """Pure rotation, the true inliers (the table of the issue): R is recovered and the median
    angle shows that there is no baseline."""
    c, x1, x2, mk, r = fitted("rot", seed, mask="true")
    Rt, _ = truth(c)
    assert r["stat"][0] == 0
    assert rot_angle_deg(r["R"].reshape(3, 3), Rt) < 0.5
    assert pose_ref.key_to_degrees(r["median_key"]) < 0.5
    assert r["stat"][6] == 0                    # n_wide at 2 degrees


@pytest.mark.parametrize("kind", tv.KINDS)
@pytest.mark.parametrize("seed", SEEDS[:2])
def test_E_against_numpy(kind, seed):
    c, x1, x2, mk, r = fitted(kind, seed)
    N = pose_ref.normal_matrix(x1, x2, mk)
    on = mk.astype(bool)
    A = np.stack([x2[on, 0] * x1[on, 0], x2[on, 0] * x1[on, 1], x2[on, 0],
                  x2[on, 1] * x1[on, 0], x2[on, 1] * x1[on, 1], x2[on, 1],
                  x1[on, 0], x1[on, 1], np.ones(on.sum())], 1)
    np.testing.assert_allclose(N, A.T @ A, rtol=1e-12, atol=1e-12)
    w, V = np.linalg.eigh(N)
    e = V[:, 0]
    tol = 100.0 * 2.0 ** -52 * w[-1] / (w[1] - w[0])   # conditioning of the null vector
    d = min(np.abs(r["E"] - e).max(), np.abs(r["E"] + e).max())
    assert d < tol, (d, tol)
    assert abs(np.linalg.norm(r["E"]) - 1.0) < 1e-14


@pytest.mark.parametrize("kind", tv.KINDS)
@pytest.mark.parametrize("seed", SEEDS)
def test_rotation_is_proper(kind, seed):
    r = fitted(kind, seed)[4]
    Rm = r["R"].reshape(3, 3)
    assert r["stat"][0] == 0
    assert np.abs(Rm.T @ Rm - np.eye(3)).max() < 1e-12
    assert abs(np.linalg.det(Rm) - 1.0) < 1e-12
    assert abs(np.linalg.norm(r["t"]) - 1.0) < 1e-12


def _numpy_vote(x1, x2):
    """incremental.relative_pose's four candidates and the depths' signs by least squares."""
    a1 = np.c_[x1, np.ones(len(x1))]
    b = np.c_[x2, np.ones(len(x2))]
    best = None
    for Rm, t in incremental.relative_pose(x1, x2):
        a = a1 @ Rm.T
        n = 0
        for ai, bi in zip(a, b):
            lam = np.linalg.lstsq(np.stack([ai, -bi], 1), -t, rcond=None)[0]
            n += bool(lam[0] > 0 and lam[1] > 0)
        if best is None or n > best[0]:
            best = (n, Rm, t)
    return best


@pytest.mark.parametrize("seed", SEEDS)
def test_winner_agrees_with_relative_pose_and_a_numpy_vote(seed):
    c, x1, x2, mk, r = fitted("general", seed)
    on = mk.astype(bool)
    n, Rm, t = _numpy_vote(x1[on], x2[on])
    assert n == r["stat"][2 + r["stat"][1]]
    assert rot_angle_deg(r["R"].reshape(3, 3), Rm) < 1e-6
    assert vec_angle_deg(r["t"], t) < 1e-6


def test_status_and_inlier_floor():
    c, x1, x2, mk, _ = fitted("general", 0, mask="true")
    idx = np.nonzero(mk)[0]
    for n, status in ((7, 1), (8, 0)):
        m = np.zeros_like(mk)
        m[idx[:n]] = 1
        r = pose_ref.pose(x1, x2, m, min_inliers=0)
        assert r["stat"][0] == status
        if status:
            assert not r["stat"][1:].any() and not r["E"].any() and not r["R"].any()
            assert not r["t"].any() and r["median_key"] == 0.0
    m = np.zeros_like(mk)
    m[idx[:14]] = 1
    assert pose_ref.pose(x1, x2, m, min_inliers=15)["stat"][0] == 1
    assert pose_ref.pose(x1, x2, m, min_inliers=14)["stat"][0] == 0
    # the batch's inl_count decides, e.g. -1 for a pair below 8 matches
    assert pose_ref.pose(x1, x2, mk, inl_count=-1)["stat"][0] == 1


@pytest.mark.parametrize("n", [20, 21])
def test_lower_median_even_and_odd(n):
    c, x1, x2, mk, full = fitted("general", 1, mask="true")
    idx = np.nonzero(mk)[0]
    m = np.zeros_like(mk)
    m[idx[:n]] = 1
    r = pose_ref.pose(x1, x2, m)
    st = r["stat"]
    assert st[0] == 0 and st[2 + st[1]] == n      # every inlier in front
    # the keys by numpy under the returned pose
    Rm, t = r["R"].reshape(3, 3), r["t"]
    a = np.c_[x1[idx[:n]], np.ones(n)] @ Rm.T
    b = np.c_[x2[idx[:n]], np.ones(n)]
    s = np.sum(np.cross(a, b) ** 2, 1) / (np.sum(a * a, 1) * np.sum(b * b, 1))
    keys = np.sort(s.astype(np.float32))
    k = (n - 1) // 2
    ulp = 2.0 ** -23 * float(keys[k + 1])
    assert float(keys[k + 1]) - float(keys[k]) > 4 * ulp   # the two middle keys are apart
    # numpy's f64 value differs from the spec's by rounding only: one f32 ulp at the most
    assert abs(float(r["median_key"]) - float(keys[k])) <= ulp
    assert st[6] == int((keys > pose_ref.wide_key(2.0)).sum())


def test_wide_key_is_the_library_value():
    for deg in (0.0, 1.0, 2.0, 45.0, 90.0):
        assert pose_ref.wide_key(deg) == sfmcore.angle_key(deg)
        assert abs(gv.key_to_degrees(float(sfmcore.angle_key(deg))) - deg) < 1e-3
    assert gv.key_to_degrees(2.0 - 0.25) == pytest.approx(150.0)
