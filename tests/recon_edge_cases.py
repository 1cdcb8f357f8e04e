"""Seeded edge cases for triangulation, the pose log map and next-view registration, shared by the
CPU tests (test_recon_hp_cpu.py) and the GPU tests (test_gpu_triangulate_edges.py, test_gpu_ba_lm.py,
test_gpu_register.py); numpy + tests/hp_ref.py (50-digit references, cached here per case).

Triangulation cases (tri_case(name) -> cams [n_cam,8], pp [n_cam,2], pt_ptr, cam_idx, uv):
  "narrow"  five ray-angle classes 30, 5, 1, 0.2, 0.05 degrees x 64 points (320: one full block of
            256 threads and a partial one); per class 6 camera centres on the rim of a cone of
            that aperture, 8 away from points in [-1,1]^3; 2- or 3-view tracks, f = 1000,
            k1 in +-0.02, |r| in 0.05..0.1, 0.5 px noise
  "ragged"  track lengths 2, 3, 4, 7, 33, 64, 65, 150 (three times) with 0- and 1-observation
            tracks between them and at both ends; a track's cameras in random order; 160 cameras
            of which the last 8 are used by no track
  "status"  exactly representable inputs: r = 0, f = 1024, centres (0,0,0), (1,0,0), (0,2,0):
            parallel rays (status 2, 2 and 3 views), rays meeting at (0.5, 0, -5) (status 3) and at
            (0.5, 0, 10) (status 0)
  "rotmat"  cameras with r = 0, |r| = 1e-11 and |r| = 2e-10 (both sides of |r|^2 = 1e-20) on a
            5-degree cone, 32 points
  "single"  one point, two cameras

Tolerances (check_triangulation):
  points    |X - X_ref|_inf <= K eps kappa (1 + |X_ref|^2), kappa = lam4 / (lam2 - lam1) from the
            reference's eigenvalues of M: the eigenvector's first-order sensitivity to a relative
            perturbation eps of M, dehomogenised.
            K = 4 x the worst ratio that oracle/recon.py (numpy.linalg.eigh, float64) shows against
            the 50-digit reference over all the cases above.  Measured (test_recon_hp_cpu.py
            prints it): per case narrow 0.867, ragged 0.519, status 0.047, rotmat 0.641, single
            0.105; hence EIGH_RATIO = 0.87 and K = 4 x 0.87 = 3.48.  The factor 4 is for the
            different summation order of M, not looseness: a numpy port of the kernel's Jacobi
            measured 0.02-0.36 on the same cases, and the same port stopped after 3 sweeps is
            1e10 outside (and changes a status).
  stats     the reference's statistics evaluated in float64 at X_ref and X_ref +- tau e_i (tau the
            point tolerance): twice the largest deviation, plus a rounding floor of 1e-9 px
            (error), 1e-12 |depth| (depth), (180/pi) 16 eps / sin(angle_ref) degrees (angle)
  status    equal for every point; fair because every generated point has |depth_min| > 1e-6 and
            |h3|/|h| < 1e-14 or > 1e-9 in the reference (asserted in tri_reference)
"""
from __future__ import annotations

import functools

import numpy as np

import hp_ref

EPS = float(np.finfo(np.float64).eps)
EIGH_RATIO = 0.87         # worst |X_eigh - X_ref| / (eps kappa (1 + |X_ref|^2)), measured
K = 4 * EIGH_RATIO
PP = (960.0, 540.0)
TRI_CASES = ("narrow", "ragged", "status", "rotmat", "single")
NARROW_DEG = (30.0, 5.0, 1.0, 0.2, 0.05)
RAGGED_LENGTHS = (2, 3, 4, 7, 33, 64, 65, 150)


def _rotmat(r):
    return hp_ref.to_f64(hp_ref.rotmat(r))


def _project(cam, pp, X):
    P = _rotmat(cam[:3]) @ X + cam[3:6]
    q = P[:2] / P[2]
    return cam[6] * (1.0 + cam[7] * (q @ q)) * q + pp


def _cone_cameras(rng, aperture_deg, rnorms, f=1000.0, k1_range=0.02):
    """One camera per entry of rnorms: centre 8 away from the origin on the rim of the cone of
    the given full aperture about -z (evenly spaced azimuths, jittered), rotation vector of the
    given norm in a random direction, so the camera looks along ~+z at the origin."""
    n = len(rnorms)
    half = np.radians(aperture_deg) / 2
    cams = np.zeros((n, 8))
    for i, rn in enumerate(rnorms):
        az = 2 * np.pi * (i + rng.uniform(-0.15, 0.15)) / n
        C = 8.0 * np.array([np.sin(half) * np.cos(az), np.sin(half) * np.sin(az), -np.cos(half)])
        d = rng.normal(size=3)
        cams[i, :3] = rn * d / np.linalg.norm(d)
        cams[i, 3:6] = -_rotmat(cams[i, :3]) @ C
        cams[i, 6] = f
        cams[i, 7] = rng.uniform(-k1_range, k1_range)
    return cams


def _observe(rng, cams, pp, tracks, X, noise):
    """tracks: list of camera-index lists (empty and single ones allowed, their point unused)."""
    ptr, ci, uv = [0], [], []
    for cs, x in zip(tracks, X):
        for c in cs:
            ci.append(c)
            uv.append(_project(cams[c], pp[c], x) + rng.normal(0.0, noise, size=2))
        ptr.append(len(ci))
    return dict(cams=cams, pp=pp, pt_ptr=np.asarray(ptr, np.int32),
                cam_idx=np.asarray(ci, np.int32), uv=np.asarray(uv, np.float64).reshape(-1, 2))


def _narrow(seed=0):
    rng = np.random.default_rng(seed)
    cams, tracks = [], []
    for k, deg in enumerate(NARROW_DEG):
        cams.append(_cone_cameras(rng, deg, rng.uniform(0.05, 0.1, size=6)))
        for p in range(64):
            views = rng.choice(6, size=2 + (p % 2), replace=False)
            tracks.append((6 * k + views).tolist())
    cams = np.concatenate(cams)
    pp = np.tile(PP, (len(cams), 1))
    X = rng.uniform(-1.0, 1.0, size=(len(tracks), 3))
    return _observe(rng, cams, pp, tracks, X, 0.5)


def _ragged(seed=1):
    rng = np.random.default_rng(seed)
    n_cam, n_used = 160, 152
    cams = np.zeros((n_cam, 8))
    for c in range(n_cam):                      # cameras 8 away looking at the origin from within
        d = rng.normal(size=3)                  # ~0.6 rad of -z
        cams[c, :3] = rng.uniform(0.05, 0.6) * d / np.linalg.norm(d)
        cams[c, 3:6] = np.array([0.0, 0.0, 8.0]) + rng.normal(0.0, 0.2, size=3)
        cams[c, 6] = 1000.0
        cams[c, 7] = rng.uniform(-0.02, 0.02)
    pp = np.tile(PP, (n_cam, 1)) + rng.uniform(-5, 5, size=(n_cam, 2))
    lengths = [0, 1]
    for rep in range(3):
        for L in RAGGED_LENGTHS:
            lengths += [L, rep % 2] if L in (3, 33, 150) else [L]
    lengths += [1, 0]
    tracks = [rng.permutation(n_used)[:L].tolist() for L in lengths]
    assert any(t != sorted(t) for t in tracks)
    X = rng.uniform(-1.0, 1.0, size=(len(tracks), 3))
    return _observe(rng, cams, pp, tracks, X, 0.5)


def _status():
    cams = np.zeros((3, 8))
    cams[:, 3:6] = -np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 2.0, 0]])   # R = I: t = -C
    cams[:, 6] = 1024.0
    pp = np.tile(PP, (3, 1))
    par = np.array(PP) + (128.0, -64.0)
    off = lambda d: np.array(PP) + (d, 0.0)
    tracks = [[0, 1], [0, 1], [0, 1, 2], [0, 1]]
    uv = [par, par, off(-102.4), off(102.4), par, par, par, off(51.2), off(-51.2)]
    return dict(cams=cams, pp=pp, pt_ptr=np.array([0, 2, 4, 7, 9], np.int32),
                cam_idx=np.array(sum(tracks, []), np.int32), uv=np.array(uv))


STATUS_EXPECTED = (2, 3, 2, 0)


def _rotmat_branches(seed=3):
    rng = np.random.default_rng(seed)
    cams = _cone_cameras(rng, 5.0, [0.0, 1e-11, 2e-10, 0.0, 1e-11, 2e-10])
    pp = np.tile(PP, (6, 1))
    tracks = [rng.choice(6, size=2 + (p % 2), replace=False).tolist() for p in range(32)]
    X = rng.uniform(-1.0, 1.0, size=(32, 3))
    return _observe(rng, cams, pp, tracks, X, 0.5)


def _single(seed=4):
    rng = np.random.default_rng(seed)
    cams = _cone_cameras(rng, 10.0, [0.07, 0.09])
    return _observe(rng, cams, np.tile(PP, (2, 1)), [[1, 0]], rng.uniform(-1, 1, size=(1, 3)), 0.5)


@functools.lru_cache(maxsize=None)
def tri_case(name):
    return dict(narrow=_narrow, ragged=_ragged, status=_status, rotmat=_rotmat_branches,
                single=_single)[name]()


@functools.lru_cache(maxsize=None)
def tri_reference(name):
    """hp_ref.triangulate of the case, solved once per process; asserts that no point of the case
    sits on a status threshold, so that statuses can be compared exactly."""
    c = tri_case(name)
    ref = hp_ref.triangulate(c["cams"], c["pp"], c["pt_ptr"], c["cam_idx"], c["uv"])
    st = ref["stats"][:, 3]
    live = st != 1
    assert np.all((ref["ratio"][live] < 1e-14) | (ref["ratio"][live] > 1e-9)), name
    solved = (st == 0) | (st == 3)
    assert np.all(np.abs(ref["stats"][solved, 2]) > 1e-6), name
    for v in ref.values():
        v.setflags(write=False)
    return ref


def point_tol(ref):
    """K eps kappa (1 + |X_ref|^2) per point (inf where there is no point to compare)."""
    lam = ref["lam"]
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = lam[:, 3] / (lam[:, 1] - lam[:, 0])
    unit = EPS * kappa * (1.0 + (ref["pts"] ** 2).sum(1))
    solved = np.isin(ref["stats"][:, 3], (0, 3))
    return np.where(solved, unit, np.inf)


def stats_tol(case, ref, tau):
    """[n, 3] tolerances on (error px, angle deg, depth) propagated from the point tolerance."""
    n = len(tau)
    out = np.zeros((n, 3))
    for p in np.nonzero(np.isin(ref["stats"][:, 3], (0, 3)))[0]:
        sl = slice(int(case["pt_ptr"][p]), int(case["pt_ptr"][p + 1]))
        f = lambda X: hp_ref.stats_f64(case["cams"], case["pp"], case["cam_idx"][sl],
                                       case["uv"][sl], X)
        s0 = f(ref["pts"][p])
        dev = np.zeros(3)
        for i in range(3):
            for sgn in (-1.0, 1.0):
                X = ref["pts"][p].copy()
                X[i] += sgn * tau[p]
                dev = np.maximum(dev, np.abs(f(X) - s0))
        sin_a = np.sin(np.radians(ref["stats"][p, 1]))
        floor = np.array([1e-9, np.degrees(16 * EPS / sin_a), 1e-12 * abs(ref["stats"][p, 2])])
        out[p] = 2.0 * dev + floor
    return out


def check_triangulation(name, pts, stats, k=K, sel=None):
    """Asserts pts / stats (rows sel of the case, default all) against the 50-digit reference.
    Returns the worst point error in units of eps kappa (1 + |X_ref|^2)."""
    case, ref = tri_case(name), tri_reference(name)
    sel = np.arange(len(ref["pts"])) if sel is None else np.asarray(sel)
    rs = ref["stats"][sel]
    np.testing.assert_array_equal(stats[:, 3], rs[:, 3], err_msg=f"{name}: status")
    dead = np.isin(rs[:, 3], (1, 2))
    assert np.all(pts[dead] == 0.0) and np.all(stats[dead, :3] == 0.0), f"{name}: dead rows not zero"
    unit = point_tol(ref)
    err = np.abs(pts - ref["pts"][sel]).max(1)
    ratio = np.where(dead, 0.0, err / unit[sel])
    worst = float(ratio.max()) if len(ratio) else 0.0
    print(f"{name}: worst point error {worst:.3f} x eps kappa (1+|X|^2) at point "
          f"{int(sel[ratio.argmax()]) if len(ratio) else -1}; allowed {k:.2f}")
    assert worst <= k, f"{name}: point error {worst:.3g} > {k:.3g} (eps kappa (1+|X|^2) units)"
    st = _stats_tol_cached(name, float(k))[sel]
    ds = np.abs(stats[:, :3] - rs[:, :3])
    # stats columns are (error, angle, depth); stats_tol columns likewise
    bad = np.nonzero((ds > st) & ~dead[:, None])
    assert len(bad[0]) == 0, (f"{name}: statistics outside tolerance at {list(zip(*bad))[:5]}: "
                              f"{ds[bad][:5]} > {st[bad][:5]}")
    return worst


@functools.lru_cache(maxsize=None)
def _stats_tol_cached(name, k):
    ref = tri_reference(name)
    tau = np.where(np.isfinite(point_tol(ref)), k * point_tol(ref), 0.0)
    return stats_tol(tri_case(name), ref, tau)


# ---- pose log map ---------------------------------------------------------------------------------

PI_DELTAS = (0.0, 1e-12, 1e-10, 1e-9, 1e-8, 5e-8, 1e-7, 1.9e-7, 2.1e-7, 1e-6, 1e-5, 1e-3, 3e-2)
PLAIN_THETAS = (0.0, 1e-12, 1e-9, 1.9e-7, 2.1e-7, 1e-6, 0.3, 1.0, 2.5)
LOGMAP_TOL = 1e-12


def axes(n_random=8, seed=5):
    rng = np.random.default_rng(seed)
    a = [np.array(e, np.float64) for e in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]
    for _ in range(n_random):
        d = rng.normal(size=3)
        a.append(d / np.linalg.norm(d))
    return a


def logmap_thetas():
    """[(label, theta as a 50-digit number)]: pi -+ delta and the plain angles."""
    import mpmath as mp
    with mp.workdps(hp_ref.DPS):
        out = []
        for d in PI_DELTAS:
            for sgn in ((-1, 1) if d > 0 else (1,)):
                out.append((f"pi{'+' if sgn > 0 else '-'}{d:g}", mp.pi + sgn * mp.mpf(d)))
        out += [(f"{t:g}", mp.mpf(t)) for t in PLAIN_THETAS]
        return out


@functools.lru_cache(maxsize=None)
def logmap_cases():
    """[(label, R float64 [3,3] rounded from the 50-digit matrix, that 50-digit matrix)]."""
    out = []
    for label, th in logmap_thetas():
        for i, a in enumerate(axes()):
            R = hp_ref.exp_so3(a, th)
            out.append((f"theta={label} axis#{i}", hp_ref.to_f64(R), R))
    return out


@functools.lru_cache(maxsize=None)
def half_turn_update():
    """cams [n,8], dc [n,8] and the 50-digit products rotmat(dc) rotmat(r), for compositions that
    land at pi -+ delta: r = a (pi -+ delta - s), dr = a s, s = 1e-2, axes e_x, e_y, e_z (every
    choice of the largest-diagonal column) and three random ones."""
    s = 1e-2
    rng = np.random.default_rng(6)
    cams, dc = [], []
    for d in PI_DELTAS:
        for sgn in ((-1.0, 1.0) if d > 0 else (1.0,)):
            for a in axes(3):
                cams.append(np.r_[a * (np.pi + sgn * d - s), rng.normal(size=5)])
                dc.append(np.r_[a * s, rng.normal(size=5) * 1e-2])
    cams, dc = np.array(cams), np.array(dc)
    ref = [hp_ref.matmul(hp_ref.rotmat(dc[c, :3]), hp_ref.rotmat(cams[c, :3]))
           for c in range(len(cams))]
    return cams, dc, ref


# ---- next-view registration -------------------------------------------------------------------------

REG_N_HYP, REG_THR, REG_SEED = 256, 3.0, 42
REG_INTR = np.array([1000.0, 0.02, 960.0, 540.0])


def _reg_image(rng, R, X, outlier_frac=0.3):
    """Noise-free projections of X under rotation R (depths >= 8), a fraction replaced by
    uniform outliers."""
    t = rng.normal(size=3)
    t = t + np.array([0, 0, 8 - (X @ R.T + t)[:, 2].min()])
    P = X @ R.T + t
    q = P[:, :2] / P[:, 2:]
    xy = REG_INTR[0] * (1 + REG_INTR[1] * (q * q).sum(1, keepdims=True)) * q + REG_INTR[2:]
    out = rng.random(len(X)) < outlier_frac
    xy[out] = rng.uniform([0, 0], [1920, 1080], size=(int(out.sum()), 2))
    return dict(R=R, t=t, X=X, xy=xy, intr=REG_INTR)


@functools.lru_cache(maxsize=None)
def reg_pose_images():
    """Images whose true rotation is I, exp(3e-9 a) and a half turn less 1e-8 / 3e-7: the RANSAC
    winner's rotation then has sin(theta) from ~1e-13 to ~3e-7, every branch of the log map."""
    import mpmath as mp
    rng = np.random.default_rng(7)
    ax = axes(1, seed=8)
    with mp.workdps(hp_ref.DPS):
        rots = [hp_ref.exp_so3(ax[0], 0), hp_ref.exp_so3(ax[3], mp.mpf(3e-9))]
        rots += [hp_ref.exp_so3(a, mp.pi - mp.mpf(1e-8)) for a in ax]
        rots += [hp_ref.exp_so3(ax[3], mp.pi - mp.mpf(3e-7))]
    return [_reg_image(rng, hp_ref.to_f64(R), rng.uniform(-2, 2, size=(200, 3))) for R in rots]


@functools.lru_cache(maxsize=None)
def reg_degenerate_images():
    """[(kind, image)]: good images around 40 collinear and 10 coincident 3-D points (no valid
    hypothesis: count -1, key -1), planar structure (z = 0), n = 3 and n = 4."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(9)
    rnd = lambda: Rotation.random(random_state=int(rng.integers(1 << 30))).as_matrix()
    box = lambda n: rng.uniform(-2, 2, size=(n, 3))
    # exactly collinear in float64: power-of-two direction components and integer steps make the
    # sample's cross product cancel to exactly 0, which is what the spec's frame test asks (n3 > 0)
    line = (np.array([0.25, -0.5, 1.0])
            + np.arange(-20, 20)[:, None] * np.array([0.125, 0.25, -0.0625]))
    same = np.tile([[0.5, -0.25, 1.0]], (10, 1))
    plane = box(100)
    plane[:, 2] = 0.0
    return [("good", _reg_image(rng, rnd(), box(120))),
            ("collinear", _reg_image(rng, rnd(), line, 0.0)),
            ("good", _reg_image(rng, rnd(), box(60))),
            ("coincident", _reg_image(rng, rnd(), same, 0.0)),
            ("planar", _reg_image(rng, rnd(), plane)),
            ("n3", _reg_image(rng, rnd(), box(3), 0.0)),
            ("n4", _reg_image(rng, rnd(), box(4), 0.0)),
            ("good", _reg_image(rng, rnd(), box(80)))]
