"""Seeded cases, tolerances and checks for the two-view pose batch (sfm_two_view_pose_batch,
csrc/two_view_pose.hip) against the 50-digit references of tests/hp_ref.py; shared by the CPU test
(test_two_view_pose_hp_cpu.py: tests/pose_ref.c and the restatement hp_ref.pose_f64) and the GPU
test (test_gpu_two_view_pose_hp.py).  Cases and references are built once per process.

Every pose case is f32 keypoints with intr = (1, 0, 0, 0), so the kernel's table holds exactly the
chosen f32-representable normalised coordinates; the "distort" family has real intrinsics.  The
reference always starts from pose_ref.undistort of the same inputs.

  fit      gen8 … gen300   generic scene (rotation 0.15, baseline 1, depth 4-8), 0.5 px noise, 8, 9,
                           15, 64, 65, 256, 257, 300 inliers
           exact8/15/64    the same without noise: a true E as closely as f32 allows
           wide            |x| up to 1.5
           patch1/2/3      every feature inside 0.1, 0.01, 0.001 of the image (and of the depth)
           planar          a plane with 1e-3 relief (small gap lam2 - lam1)
           base1 … base4   baseline 1e-1 … 1e-4 of the depth
           forward         forward motion, epipole inside the image
           rotation        no baseline;  identical: x1 = x2
  decomp   junk8/20/64     random matches
           rank1           half the matches with x2 on a line, half with x1 on a line: the only
                           null vector is the rank-one l2 l1^T, status 2 through the public entry
           lines           every x1 on a line and every x2 on a line (a 5-dimensional null space:
                           whichever vector Jacobi returns)
           near_rank1      rank1 with the lines blurred by 1e-2 (sigma2 / sigma1 = 3e-3)
  vote     depth           100 points at 1 … 1e4 baselines, one at 1e5, one at 1e6
           baseline        forward motion, one of 64 points on the baseline
           behind          points behind the first and behind both cameras
           wide90          rays up to ~110 degrees apart (a.b < 0, the 2 - s branch)
           zero_front      8 random matches no candidate puts in front;  tie: the vote ties
           wk_eq/lo/hi     one scene, wide_key equal to a match's key and the two f32 neighbours
           med_even/odd    22 / 23 in front with equal middle keys
  distort  d1 … d3         f = 1000, 1920x1080, k1 pairs (0.3, -0.1), (0.02, -0.02), (-0.05, 0.1)
  shape    (byte parity only) M in 255 … 513 with the inliers last; k_max 1, 8, 8192; counts above
           k_max and below 0, match and image ids out of range
  undistortion  k1 in 0, ±1e-3, ±0.02, ±0.05, ±0.1, ±0.3 at the centre, mid-image and the corner

Units.  N: eps sum |terms| per entry.  E: eps lam9 / (lam2 - lam1) of the exact N.  R, t:
eps sigma1 / (sigma2 - sigma3) of the code's own E.  l1, l2, key: the first-order float64 error of
their evaluation (hp_ref.VU).  Undistortion: (eps + rho^10) |x|, rho the contraction factor.
Each K is 4 x the worst ratio of LAPACK / plain numpy float64 on the same cases (LAPACK_RATIO,
measured by test_lapack_ratios_behind_every_K); the code under test never sets a K.

Measured (the tests print every ratio per case), worst over the cases, tests/pose_ref.c and the
kernels on an MI355X alike (the same bytes), next to numpy / LAPACK and K:
  N      1.10 (patch1)       numpy 6.70 (gen256)   K 26.8
  E      0.094 (wide)        eigh  0.254 (junk20)  K 1.02
  R, t   18.5 (near_rank1), <= 4.5 elsewhere      svd 34.5 (gen15)   K 138
  l1/l2  0.231 (depth)       numpy 0.203 (exact64) K 0.812; excused: the point on the baseline only
  orth   9.0 eps (gen65), |E| - 1 5.8 eps (identical)   K_ORTH 16
  undistortion vs the same steps in 50 digits 0.231 of their unit; vs the true inverse 0.469 of
  (eps + rho^10) |x| (numpy the same, K 1.88); pixel errors per (k1, position) in DESIGN §4.2b
  E vs the null vector of A (reported): 0.07-4.6 units on generic cases, 930 / 6.6e4 at a 0.01 /
  0.001 patch, 1.3e3 at a 1e-4 baseline
Each of the eight mutations of hp_ref.pose_f64 fails its case of MUTATION_CASES: a, b, c leave E
2e11 units off, d leaves R^T R - I at 91 eps, e empties the winner's count, f, g move the median,
h moves n_wide.  The restatement itself passes every case.  Nothing was found in the kernels; found
in the test infrastructure: pref_pose_batch did not clamp ids and counts as the kernels do.
"""
from __future__ import annotations

import functools

import numpy as np

import hp_ref
import pose_ref

EPS = hp_ref.EPS
UNIT_INTR = np.array([1.0, 0.0, 0.0, 0.0])
REAL_INTR = np.array([1000.0, 0.0, 960.0, 540.0])

# worst ratio of numpy.linalg.eigh / svd and plain numpy float64 sums against the 50-digit reference
# over all cases, each in its unit (test_lapack_ratios prints and pins them), and K = 4 x that
LAPACK_RATIO = dict(N=6.70, E=0.254, R=34.5, V=0.203, U=0.469)
K_N = 4 * LAPACK_RATIO["N"]      # 26.8   A.T @ A (gen256)
K_E = 4 * LAPACK_RATIO["E"]      # 1.02   numpy.linalg.eigh of it (junk20)
K_R = 4 * LAPACK_RATIO["R"]      # 138    numpy.linalg.svd of the spec's own E (gen15)
K_V = 4 * LAPACK_RATIO["V"]      # 0.812  matrix products and einsum (exact64)
K_U = 4 * LAPACK_RATIO["U"]      # 1.88   the ten steps on numpy arrays (k1 = 0.02, mid-image)
# "a few eps" for R^T R - I, det R - 1, |t| - 1 and |E| - 1: U is orthonormal to the roundings of
# one normalisation and one Gram-Schmidt step per column (~4 eps), V to those of the ~12 plane
# rotations a 3x3 Jacobi accumulates (each ~1 eps, adding in quadrature: ~4 eps); twice their sum
K_ORTH = 16
# pose_ref.undistort against the same 10 steps in 50 digits, in the steps' own first-order unit
K_STEPS = 1.0
EXCUSED_CAP = 0.02

UNDISTORT_K1 = (0.0, 1e-3, -1e-3, 0.02, -0.02, 0.05, -0.05, 0.1, -0.1, 0.3, -0.3)
UNDISTORT_POS = dict(centre=(960.0, 540.0), mid=(1440.0, 810.0), corner=(1920.0, 1080.0))

GEN_SIZES = (8, 9, 15, 64, 65, 256, 257, 300)
# seeds found by a search over random 8-match sets (tests/pose_hp_cases.py: _junk)
ZERO_FRONT_SEED = 232598
TIE_SEED = 13

MUTATION_CASES = dict(a="gen64", b="exact64", c="gen64", d="near_rank1", e="gen64", f="wide90",
                      g="gen64", h="wk_eq")


def _rot(axis, ang):
    return hp_ref.rotmat_f64(np.asarray(axis, np.float64) / np.linalg.norm(axis) * ang)[0]


def _lookat(C, target):
    z = np.asarray(target, np.float64) - C
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


R_GEN = _rot((0.3, 1.0, 0.2), 0.15)


def _views(X, R, C, rng=None, noise=0.0):
    x1 = X[:, :2] / X[:, 2:]
    P = (X - np.asarray(C, np.float64)) @ R.T
    x2 = P[:, :2] / P[:, 2:]
    if noise:
        x1 = x1 + rng.normal(0.0, noise, x1.shape)
        x2 = x2 + rng.normal(0.0, noise, x2.shape)
    return x1.astype(np.float32), x2.astype(np.float32)


def _cloud(rng, n, depth=(4.0, 8.0), centre=(0.0, 0.0), half=0.6):
    x = np.asarray(centre) + rng.uniform(-half, half, (n, 2))
    z = rng.uniform(*depth, n)
    return np.c_[x * z[:, None], z]


def _case(name, family, kp1, kp2, **kw):
    c = dict(name=name, family=family, kp1=np.ascontiguousarray(kp1, np.float32),
             kp2=np.ascontiguousarray(kp2, np.float32), intr1=UNIT_INTR, intr2=UNIT_INTR,
             min_angle_deg=2.0, loose=False, status=0, vote=True)
    c.update(kw)
    c.setdefault("mask", np.ones(len(c["kp1"]), np.uint8))
    c["x1"] = pose_ref.undistort(c["kp1"], c["intr1"])
    c["x2"] = pose_ref.undistort(c["kp2"], c["intr2"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _junk(seed, n):
    rng = np.random.default_rng([seed, n])
    return rng.uniform(-1, 1, (n, 2)).astype(np.float32), rng.uniform(-1, 1, (n, 2)).astype(np.float32)


def _wide_deg(key):
    """min_angle_deg whose wide_key is exactly the f32 `key`."""
    deg = float(np.degrees(np.arcsin(np.sqrt(np.float64(key)))))
    for _ in range(64):
        w = pose_ref.wide_key(deg)
        if w == key:
            return deg
        deg = float(np.nextafter(deg, np.inf if w < key else -np.inf))
    lo, hi = deg - 1e-6, deg + 1e-6
    for _ in range(200):
        deg = 0.5 * (lo + hi)
        w = pose_ref.wide_key(deg)
        if w == key:
            return deg
        lo, hi = (deg, hi) if w < key else (lo, deg)
    raise AssertionError("no angle gives this key")


def _build():
    out = []
    add = lambda *a, **k: out.append(_case(*a, **k))
    C1 = (1.0, 0.2, 0.1)
    for n in GEN_SIZES:
        rng = np.random.default_rng([1, n])
        add(f"gen{n}", "fit", *_views(_cloud(rng, n), R_GEN, C1, rng, 5e-4))
    for n in (8, 15, 64):
        rng = np.random.default_rng([2, n])
        add(f"exact{n}", "fit", *_views(_cloud(rng, n), R_GEN, C1))
    rng = np.random.default_rng(3)
    add("wide", "fit", *_views(_cloud(rng, 40, half=1.5), R_GEN, C1))
    for i, frac in enumerate((0.1, 0.01, 0.001)):
        rng = np.random.default_rng([4, i])
        X = _cloud(rng, 40, depth=(6.0 * (1 - frac), 6.0 * (1 + frac)), centre=(0.3, -0.2), half=frac)
        add(f"patch{i + 1}", "fit", *_views(X, R_GEN, C1))
    rng = np.random.default_rng(5)
    X = _cloud(rng, 40)
    X[:, 2] = 6.0 + 0.3 * X[:, 0] / X[:, 2] + rng.uniform(-1e-3, 1e-3, 40)
    X[:, :2] = rng.uniform(-0.6, 0.6, (40, 2)) * X[:, 2:]
    add("planar", "fit", *_views(X, R_GEN, C1))
    for i in range(1, 5):
        rng = np.random.default_rng([6, i])
        add(f"base{i}", "fit", *_views(_cloud(rng, 40), R_GEN, 6.0 * 10.0 ** -i * np.array(C1)))
    C_FWD = np.array([0.05, 0.02, 1.0])
    rng = np.random.default_rng(7)
    add("forward", "fit", *_views(_cloud(rng, 40), _rot((1, 0, 0), 0.02), C_FWD))
    rng = np.random.default_rng(8)
    # without a baseline every depth numerator and every key is rounding noise (each point is at
    # infinitely many baselines): the vote of these two is not compared, only fit and poses
    add("rotation", "fit", *_views(_cloud(rng, 40), R_GEN, (0.0, 0.0, 0.0)), vote=False)
    rng = np.random.default_rng(9)
    x = rng.uniform(-0.6, 0.6, (40, 2)).astype(np.float32)
    add("identical", "fit", x, x.copy(), vote=False)

    for n in (8, 20, 64):
        add(f"junk{n}", "decomp", *_junk(100, n))
    for name, blur, status in (("rank1", 0.0, 2), ("near_rank1", 1e-2, 0)):
        rng = np.random.default_rng(10)
        a, b = rng.uniform(-1, 1, (24, 2)), rng.uniform(-1, 1, (24, 2))
        b[:12, 1] = 0.25 + blur * rng.uniform(-1, 1, 12)      # x2 on the line y = 0.25
        a[12:, 0] = 0.5 + blur * rng.uniform(-1, 1, 12)       # x1 on the line x = 0.5
        add(name, "decomp", a, b, status=status)
    rng = np.random.default_rng(11)
    a, b = rng.uniform(-1, 1, (24, 2)), rng.uniform(-1, 1, (24, 2))
    a[:, 0], b[:, 1] = 0.5, 0.25
    add("lines", "decomp", a, b, status=None)

    rng = np.random.default_rng(12)
    X = _cloud(rng, 100)
    z = np.r_[np.geomspace(1.0, 1e4, 98), 1e5, 1e6]
    X = np.c_[X[:, :2] / X[:, 2:] * z[:, None], z]
    add("depth", "vote", *_views(X, R_GEN, (1.0, 0.0, 0.0)), loose=True)
    rng = np.random.default_rng(13)
    X = np.r_[_cloud(rng, 63), [3.0 * C_FWD]]
    add("baseline", "vote", *_views(X, _rot((1, 0, 0), 0.02), C_FWD), loose=True)
    rng = np.random.default_rng(14)
    X = np.r_[_cloud(rng, 40), _cloud(rng, 5, depth=(-0.3, -0.2)), _cloud(rng, 5, depth=(-8.0, -4.0))]
    add("behind", "vote", *_views(X, R_GEN, (1.0, 0.0, -0.5)))
    rng = np.random.default_rng(15)
    X = np.array([0.0, 0.0, 5.0]) + rng.uniform(-1.5, 1.5, (40, 3))
    C = np.array([6.0, 0.0, 7.0])
    add("wide90", "vote", *_views(X, _lookat(C, (0.0, 0.0, 5.0)), C))
    add("zero_front", "vote", *_junk(ZERO_FRONT_SEED, 8))
    add("tie", "vote", *_junk(TIE_SEED, 8))
    rng = np.random.default_rng(16)
    kp = _views(_cloud(rng, 21), R_GEN, C1)
    k0 = _key_of(kp, 7)
    for name, k in (("wk_eq", k0), ("wk_lo", np.nextafter(k0, np.float32(0))),
                    ("wk_hi", np.nextafter(k0, np.float32(2)))):
        add(name, "vote", *kp, min_angle_deg=_wide_deg(k), key0=k0)
    rng = np.random.default_rng(17)
    a, b = _views(_cloud(rng, 21), R_GEN, C1)
    mid = _middle(a, b)
    rest = [i for i in range(21) if i != mid]
    for name, idx in (("med_even", rest[:19] + [mid] * 3), ("med_odd", rest + [mid] * 3)):
        add(name, "vote", a[idx], b[idx])

    K1S = ((0.3, -0.1), (0.02, -0.02), (-0.05, 0.1))
    for i, (ka, kb) in enumerate(K1S):
        rng = np.random.default_rng([18, i])
        x1, x2 = _views(_cloud(rng, 64, half=0.9), R_GEN, C1)
        ia, ib = REAL_INTR.copy(), REAL_INTR.copy()
        ia[1], ib[1] = ka, kb
        dist = lambda x, it: (it[0] * x.astype(np.float64)
                              * (1.0 + it[1] * (x.astype(np.float64) ** 2).sum(1, keepdims=True))
                              + it[2:])
        add(f"d{i + 1}", "distort", dist(x1, ia), dist(x2, ib), intr1=ia, intr2=ib)
    return {c["name"]: c for c in out}


def _key_of(kp, m):
    """The f32 key of match m under pose_ref's own pose of the scene."""
    x1, x2 = kp[0].astype(np.float64), kp[1].astype(np.float64)
    r = pose_ref.pose(x1, x2, min_inliers=8)
    return hp_ref.score_f64(r["R"], r["t"], x1, x2)[2][m]


def _middle(a, b):
    """The match whose key is the median of the scene under pose_ref's pose."""
    x1, x2 = a.astype(np.float64), b.astype(np.float64)
    r = pose_ref.pose(x1, x2, min_inliers=8)
    return int(np.argsort(hp_ref.score_f64(r["R"], r["t"], x1, x2)[2], kind="stable")[len(a) // 2])


@functools.lru_cache(maxsize=None)
def cases():
    return _build()


def case(name):
    return cases()[name]


def names(family=None):
    return [n for n, c in cases().items() if family is None or c["family"] == family]


FAMILIES = ("fit", "decomp", "vote", "distort")


def batches():
    """[(label, [case names], min_angle_deg)]: one batch per family; the wide_key cases need a
    call each, since min_angle_deg belongs to the call."""
    out = []
    for fam in FAMILIES:
        by_angle = {}
        for n in names(fam):
            by_angle.setdefault(case(n)["min_angle_deg"], []).append(n)
        for deg, ns in by_angle.items():
            out.append((fam if deg == 2.0 else f"{fam}@{ns[0]}", ns, deg))
    return out


def batch_args(ns):
    """The batch's host arrays for the cases `ns`: two images per case, identity matches."""
    cs = [case(n) for n in ns]
    k_max = max(len(c["kp1"]) for c in cs)
    P = len(cs)
    kps = np.zeros((2 * P, k_max, 2), np.float32)
    intr = np.zeros((2 * P, 4))
    match = np.zeros((P, k_max, 2), np.int32)
    match[:, :, 0] = match[:, :, 1] = np.arange(k_max)
    mask = np.zeros((P, k_max), np.uint8)
    count = np.zeros(P, np.int32)
    for p, c in enumerate(cs):
        M = len(c["kp1"])
        kps[2 * p, :M], kps[2 * p + 1, :M] = c["kp1"], c["kp2"]
        intr[2 * p], intr[2 * p + 1] = c["intr1"], c["intr2"]
        mask[p, :M], count[p] = c["mask"], M
    pairs = np.arange(2 * P, dtype=np.int32).reshape(P, 2)
    return kps, intr, pairs, count, match, mask, mask.sum(1).astype(np.int32)


def row(res, p):
    return {k: res[k][p] for k in ("E", "R", "t", "stat", "median_key")}


# ---- references -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fit_ref(name):
    c = case(name)
    return hp_ref.pose_normal(c["x1"], c["x2"], c["mask"])


@functools.lru_cache(maxsize=None)
def _dec_ref(key):
    return hp_ref.pose_decompose(np.frombuffer(key, np.float64))


@functools.lru_cache(maxsize=None)
def _vote_ref(name, key):
    c = case(name)
    v = np.frombuffer(key, np.float64)
    return hp_ref.pose_vote(v[:9], v[9:], c["x1"], c["x2"], c["mask"])


def _inliers(c):
    on = c["mask"].astype(bool)
    return c["x1"][on], c["x2"][on]


def _fronts(l1, l2):
    return (l1 > 0) & (l2 > 0), (l1 < 0) & (l2 < 0)


def excused_by_reference(name, cand):
    """Matches the 50-digit reference alone excuses under the candidates (Ra, Rb, u3): a numerator
    within K_V units of zero."""
    ex = None
    for Rc in cand[:2]:
        v = _vote_ref(name, np.r_[Rc, cand[2]].tobytes())
        e = (np.abs(v["l1"]) <= K_V * v["u_l1"]) | (np.abs(v["l2"]) <= K_V * v["u_l2"])
        ex = e if ex is None else ex | e
    return ex


def check(name, out, label, N=None, kN=None, kE=None, kR=None):
    """Prints the ratios of one case's outputs (dict E, R, t, stat, median_key and, for a
    restatement, its own cand) and asserts them; returns the ratios."""
    c = case(name)
    x1, x2 = _inliers(c)
    n_inl = len(x1)
    ref = fit_ref(name)
    st = np.asarray(out["stat"])
    r = {}
    if N is not None:
        r["N"] = hp_ref.normal_ratio(N, ref)
        assert r["N"] <= (K_N if kN is None else kN), (name, label, "N", r["N"])
    if c["status"] is not None:
        assert st[0] == c["status"], (name, label, "status", st)
    if st[0] != 0:
        assert not np.asarray(out["E"]).any() and not np.asarray(out["R"]).any()
        assert not np.asarray(out["t"]).any() and not st[1:].any() and out["median_key"] == 0
        if c["status"] == 2:    # the 50-digit null vector is rank one as well
            e = np.array([float(x) for x in ref["e"]])
            assert hp_ref.pose_decompose(e)["status2"], (name, "the reference is not degenerate")
        print(f"{name} {label}: status {st[0]}" + "".join(f" {k}={v:.3g}" for k, v in r.items()))
        return r
    E, Rm, t = np.asarray(out["E"]), np.asarray(out["R"]), np.asarray(out["t"])
    assert np.isfinite(E).all() and np.isfinite(Rm).all() and np.isfinite(t).all()
    assert st[7] == n_inl
    # E against the null vector of the exact N, and (reported) against that of A itself
    uE = EPS * ref["lam"][8] / ref["gap"] if ref["gap"] > 0 else np.inf
    uA = EPS * ref["sv"][8] / ref["sgap"] if ref["sgap"] > 0 else np.inf
    r["E"] = hp_ref.vec_dist(E, ref["e"]) / uE
    r["A"] = hp_ref.vec_dist(E, ref["a_null"]) / uA
    r["errA"] = hp_ref.vec_dist(E, ref["a_null"])
    r["normE"] = abs(hp_ref.norm_minus_1(E)) / EPS
    assert r["E"] <= (K_E if kE is None else kE), (name, label, "E", r["E"])
    # R, t against the nearest 50-digit candidate of the code's own E
    dec = _dec_ref(E.tobytes())
    assert not dec["status2"]
    r["R"] = hp_ref.pose_dist(Rm, t, dec["cands"]) / dec["unit"]
    r["orth"] = hp_ref.orth_defect(Rm, t) / EPS
    assert r["R"] <= (K_R if kR is None else kR), (name, label, "R", r["R"], dec["sigma"])
    assert r["orth"] <= K_ORTH and r["normE"] <= K_ORTH, (name, label, "orth", r["orth"], r["normE"])
    # the vote
    cand = out.get("cand") or pose_ref.candidates(E)[:3]
    cand = tuple(np.asarray(x, np.float64).ravel() for x in cand)
    best = int(st[1])
    assert best == int(np.argmax(st[2:6])), (name, label, "winner", st)
    np.testing.assert_array_equal(Rm, cand[best >> 1])
    np.testing.assert_array_equal(t, -cand[2] if best & 1 else cand[2])
    if not c["vote"]:
        print(f"{name} {label}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items()) + "  (no vote)")
        return r
    excused = excused_by_reference(name, cand)
    n_exc = int(excused.sum())
    assert n_exc <= EXCUSED_CAP * n_inl and (c["loose"] or n_exc == 0), (name, label, "excused", n_exc)
    worstV = 0.0
    for ri, Rc in enumerate(cand[:2]):
        v = _vote_ref(name, np.r_[Rc, cand[2]].tobytes())
        l1, l2, _ = hp_ref.score_f64(Rc, cand[2], x1, x2)
        worstV = max(worstV, float(np.max(np.abs(l1 - v["l1"]) / v["u_l1"])),
                     float(np.max(np.abs(l2 - v["l2"]) / v["u_l2"])))
        for sign, (f64, hp) in enumerate(zip(_fronts(l1, l2), _fronts(v["l1"], v["l2"]))):
            keep = ~excused
            assert (f64[keep] == hp[keep]).all(), (name, label, "decision", ri, sign)
            assert st[2 + 2 * ri + sign] - int(f64[excused].sum()) == int(hp[keep].sum()), \
                (name, label, "count", 2 * ri + sign, st)
    r["V"] = worstV
    # keys of the inliers in front under the winner
    tb = -cand[2] if best & 1 else cand[2]
    v = _vote_ref(name, np.r_[cand[best >> 1], cand[2]].tobytes())
    l1, l2, key = hp_ref.score_f64(cand[best >> 1], tb, x1, x2)
    front = (l1 > 0) & (l2 > 0)
    own = np.sort(key[front])
    n = int(st[2 + best])
    wk = pose_ref.wide_key(c["min_angle_deg"])
    assert len(own) == n
    # the lower median has the right rank among the code's own keys (the spec's operations in
    # numpy float64: the code's bits), and n_wide counts them
    assert st[6] == int((own > wk).sum()), (name, label, "n_wide", st[6])
    assert np.float32(out["median_key"]) == (own[(n - 1) // 2] if n else np.float32(0)), \
        (name, label, "median", out["median_key"])
    # and against the 50-digit keys rounded once to f32
    hp_front = _fronts(v["l1"], v["l2"])[best & 1] & ~excused
    lo, hi = hp_ref.key_bracket(v["key_mp"], K_V * v["u_key"])
    r["key"] = float(np.max(np.abs(key.astype(np.float64) - v["key"])[hp_front]
                            / (v["u_key"] + 2.0 ** -24 * v["key"])[hp_front])) if hp_front.any() else 0.0
    loose_key = hp_front & ((lo != hi) | ((lo > wk) != (hi > wk)))
    assert loose_key.sum() + n_exc <= EXCUSED_CAP * n_inl and (c["loose"] or not loose_key.any())
    maybe = excused & front
    lo_all = np.r_[lo[hp_front], key[maybe]]
    hi_all = np.r_[hi[hp_front], key[maybe]]
    assert len(lo_all) == n
    assert (lo_all > wk).sum() <= st[6] <= (hi_all > wk).sum(), (name, label, "n_wide vs 50 digits")
    if n:
        med, rank = np.float32(out["median_key"]), (n - 1) // 2
        assert (hi_all < med).sum() <= rank < (lo_all <= med).sum(), (name, label, "median vs 50 digits")
    print(f"{name} {label}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items())
          + f"  front={st[2:6].tolist()} best={best} excused={n_exc}")
    return r


# ---- LAPACK / plain numpy on the same cases, in the same units -------------------------------------

def lapack_ratios(name, E=None):
    """Worst ratios of numpy.linalg.eigh / svd and plain numpy float64 sums on one case: N, E, and
    for the float64 E given (the code's own) R and V."""
    c = case(name)
    x1, x2 = _inliers(c)
    ref = fit_ref(name)
    A = np.stack([x2[:, 0] * x1[:, 0], x2[:, 0] * x1[:, 1], x2[:, 0], x2[:, 1] * x1[:, 0],
                  x2[:, 1] * x1[:, 1], x2[:, 1], x1[:, 0], x1[:, 1], np.ones(len(x1))], 1)
    N = A.T @ A
    r = dict(N=hp_ref.normal_ratio(N, ref))
    uE = EPS * ref["lam"][8] / ref["gap"] if ref["gap"] > 0 else np.inf
    r["E"] = hp_ref.vec_dist(np.linalg.eigh(N)[1][:, 0], ref["e"]) / uE
    if E is not None and np.asarray(E).any():
        dec = _dec_ref(np.asarray(E, np.float64).tobytes())
        U, S, Vt = np.linalg.svd(np.asarray(E).reshape(3, 3))
        u1, u2, v1, v2 = U[:, 0], U[:, 1], Vt[0], Vt[1]
        u3, v3 = np.cross(u1, u2), np.cross(v1, v2)
        Ra = np.outer(u2, v1) - np.outer(u1, v2) + np.outer(u3, v3)
        Rb = np.outer(u1, v2) - np.outer(u2, v1) + np.outer(u3, v3)
        r["R"] = max(hp_ref.pose_dist(Rc, u3, dec["cands"]) for Rc in (Ra, Rb)) / dec["unit"]
        cand = pose_ref.candidates(E)
        worst = 0.0
        for Rc in cand[:2]:
            v = _vote_ref(name, np.r_[Rc, cand[2]].tobytes())
            a = np.c_[x1, np.ones(len(x1))] @ Rc.reshape(3, 3).T
            b = np.c_[x2, np.ones(len(x2))]
            t = cand[2]
            ab, aa, bb = np.einsum("ij,ij->i", a, b), np.einsum("ij,ij->i", a, a), np.einsum("ij,ij->i", b, b)
            l1 = ab * (b @ t) - (a @ t) * bb
            l2 = aa * (b @ t) - ab * (a @ t)
            worst = max(worst, float(np.max(np.abs(l1 - v["l1"]) / v["u_l1"])),
                        float(np.max(np.abs(l2 - v["l2"]) / v["u_l2"])))
        r["V"] = worst
    return r


# ---- undistortion ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def undistort_table():
    """One row per (k1, position): dict k1, pos, kr2 = k1 r_d^2, rho, exists, px (pixel error of the
    spec's 10 steps against the true inverse at f = 1000), steps (ratio against the 10 steps in 50
    digits), exact (ratio in (eps + rho^10) |x|), numpy (the same ratio for plain numpy float64
    steps), x (the spec's output)."""
    rows = []
    for k1 in UNDISTORT_K1:
        intr = REAL_INTR.copy()
        intr[1] = k1
        for pos, uv in UNDISTORT_POS.items():
            kp = np.array([uv], np.float32)
            x = pose_ref.undistort(kp, intr)[0]
            xd = (kp[0].astype(np.float64) - intr[2:]) / intr[0]
            xn = xd.copy()
            for _ in range(10):
                xn = xd / (1.0 + k1 * (xn @ xn))
            d = hp_ref.undistort_compare(xd, k1, x, xn)
            d.update(k1=k1, pos=pos, kr2=k1 * float(xd @ xd), x=x)
            rows.append(d)
    return rows


# ---- shape batches (byte parity only) ---------------------------------------------------------------

def _scene_kps(rng, k_max):
    a, b = _views(_cloud(rng, k_max), R_GEN, (1.0, 0.2, 0.1), rng, 5e-4)
    return np.stack([a, b])


def _identity(P, k_max):
    m = np.zeros((P, k_max, 2), np.int32)
    m[:, :, 0] = m[:, :, 1] = np.arange(k_max)
    return m


STRIDE_M = (255, 256, 257, 511, 512, 513)


@functools.lru_cache(maxsize=None)
def shape_batches():
    """{label: (kps, intr, pairs, count, match, mask, inl_count)}."""
    out = {}
    intr2 = np.tile(UNIT_INTR, (2, 1))
    # M at the 256-stride of both kernels, the inliers in the last slots
    k_max, P = 513, len(STRIDE_M)
    mask = np.zeros((P, k_max), np.uint8)
    for p, M in enumerate(STRIDE_M):
        mask[p, M - 20:M] = 1
    out["stride"] = (_scene_kps(np.random.default_rng(30), k_max), intr2,
                     np.tile(np.array([[0, 1]], np.int32), (P, 1)), np.array(STRIDE_M, np.int32),
                     _identity(P, k_max), mask, mask.sum(1).astype(np.int32))
    # k_max = 1: too few inliers, and an inl_count that claims 8 (the fit of a single row)
    out["kmax1"] = (_scene_kps(np.random.default_rng(31), 1), intr2,
                    np.array([[0, 1], [0, 1]], np.int32), np.array([1, 1], np.int32), _identity(2, 1),
                    np.ones((2, 1), np.uint8), np.array([1, 8], np.int32))
    out["kmax8"] = (_scene_kps(np.random.default_rng(32), 8), intr2, np.array([[0, 1]], np.int32),
                    np.array([8], np.int32), _identity(1, 8), np.ones((1, 8), np.uint8),
                    np.array([8], np.int32))
    # k_max = 8192 = M: every match an inlier, and 40 inliers in the last slots
    k_max = 8192
    mask = np.ones((2, k_max), np.uint8)
    mask[1, :k_max - 40] = 0
    out["kmax8192"] = (_scene_kps(np.random.default_rng(33), k_max), intr2,
                       np.array([[0, 1], [1, 0]], np.int32), np.full(2, k_max, np.int32),
                       _identity(2, k_max), mask, mask.sum(1).astype(np.int32))
    # counts and ids outside their arrays
    k_max, P = 64, 6
    kps = np.concatenate([_scene_kps(np.random.default_rng(34), k_max),
                          _scene_kps(np.random.default_rng(35), k_max)])
    match = _identity(P, k_max)
    mask = np.ones((P, k_max), np.uint8)
    count = np.array([100, -5, 64, 64, 40, 2 ** 31 - 1], np.int32)
    pairs = np.array([[0, 1], [0, 1], [0, 1], [-1, 4], [7, -2 ** 31], [2, 3]], np.int32)
    match[2, ::5, 0] = [-3, k_max, 2 ** 31 - 1, -2 ** 31, 64, 65, -1, 1000, 63, 0, 7, -64, 128][:13]
    match[2, 1::7, 1] = [k_max, -1, 2 ** 30, -2 ** 30, 99, 64, -65, 8192, 70][:9]
    match[4, :, 1] = match[4, ::-1, 1] + 30
    mask[4, 40:] = 0
    mask[5, 1::2] = 0
    inl = np.array([64, 8, 64, 64, 40, 32], np.int32)
    out["clamps"] = (kps, np.tile(UNIT_INTR, (4, 1)), pairs, count, match, mask, inl)
    return out


def clamped(args):
    """The same batch with every id and count clamped by numpy, as DESIGN §4.2b states the rule."""
    kps, intr, pairs, count, match, mask, inl = args
    n_img, k_max, _ = kps.shape
    return (kps, intr, np.clip(pairs, 0, n_img - 1).astype(np.int32),
            np.clip(count, 0, k_max).astype(np.int32), np.clip(match, 0, k_max - 1).astype(np.int32),
            mask, inl)
