"""Seeded cases for the bundle-adjustment step solve (sfm_ba_solve, csrc/ba_solve.hip), shared by
the CPU test (test_ba_solve_hp_cpu.py) and the GPU test (test_gpu_ba_solve_hp.py); numpy,
oracle/ and tests/hp_ref.py.  Cases and their references are built once per process.

A case is a set of float64 blocks U, V, W, g_c, g_p (oracle.ba_jtj of a seeded problem, or
hand-made) with its index arrays and, for "gn", a mask of held parameters; a run is a case with
λ, tol and max_iter.  The blocks are exact inputs: the solve is checked on them, whatever
linearisation made them.  RUNS lists the runs; case(name), reference(run), measure(...) and
check(...) are the interface.

Edge cases (at most 12 cameras, about 100 points; every run at tol 1e-13, cap 500 unless said):
  benign     8 cameras x 60 points x 4 views; λ = 1e-14, 1e-8, 1e-4, 1, 1e4, 1e12; at λ = 1e-4
             also tol = 0.1 (the incremental driver's) and max_iter = 3 (the cap is hit)
  gn         λ = 0 with the gauge and the intrinsics held (reconstruction.gauge_mask through
             sfm_ba_fix_params), every point seen by 4 cameras
  fewview_px cameras holding 1, 2, 3 and 4 observations among 8 normal ones, pixel units
             (f ~ 1000) as every other case; λ = 1e-4
  fewview    the same in normalised image units (f ~ 1, see _unit_cam); λ = 1e-4, 1e-8: at
             f ~ 1000 px a camera of one observation at λ = 1e-8 has 0.04 x the SPD margin below
  single     12 points with one observation (V of rank 2) and a point seen twice by one camera;
             λ = 1e-4, 1e-10
  narrow     points seen by two cameras only whose rays are 0.05 and 0.5 degrees apart; λ = 1e-6
  clamp      a camera (f = 200) whose 4 observations lie within 1 px of its principal point, so
             U[7][7] < 1e-6 and the clamp sets its damping; an unobserved camera; unobserved points
             at both ends and in the middle; λ = 1
  zero       the benign blocks with g_c = g_p = 0: no iteration, δ = 0, info[1] = 0
  fallback   hand-made, 5 cameras, no points: SPD integer blocks, camera 2's block
             [[P, 0], [0, -1]] with P SPD and not diagonal (Cholesky pivot 7 is -1 + λ 1e-6), its
             b[7] = 0, so the negative direction is never entered; λ = 0.25.  Also at max_iter = 1,
             where dc = α M b shows the diagonal preconditioner of camera 2
  breakdown  the same with g_c[2][7] = 3: p_0 = M b has 3e6 / (1 - 2.5e-7) along the negative
             direction, p·q ~ -9e12 at iteration 0
  fallback_obs, breakdown_obs   the same two events with observations, so that the explicit
             system runs them too: the benign blocks at λ = 1e-4 with camera 7's k1 decoupled (its
             row and column of U and its rows of W zeroed, as sfm_ba_fix_params does) and
             U[7][7][7] = -1, so S_cc = [[S', 0], [0, -1 + λ 1e-6]] exactly: the same pivot, the
             same margin; g_c[7][7] = 0 (never entered) or 3 (p·q ~ -9e12 at iteration 0);
             fallback_obs also at max_iter = 1
Shape cases (benign parameters, tol 1e-12, cap 300; λ = SHAPE_LAMBDA, the smallest of 1e-3, 1e-2,
1e-1 at which the oracle converges within the cap and every S_cc has the SPD margin; no iteration
count is asserted):
  S1, S2a, S2b  ba_edge_cases.case: 6 / 260 cameras of 0 to 300 observations, tracks of 0, 1, 2, 63,
             64, 65, 150, 257, n_obs = 6 x 256 and 1499
  S3         33 cameras (the last bas_pcg_vec block holds one) of which four hold 255, 256, 257 and
             513 observations; tracks of 7, 8, 9, 31, 32, 33, 128, 129 (a camera sees a long track
             more than once); n_pt = 583 (no multiple of 32); the 129-track is the last point

Units (hp_ref.SolveRef; eps = 2^-52, all derived):
  backsub   per point, 2-norm, against δp(dc) of the SAME dc in 50 digits:
            u_p = eps (κ₂(V_d) ‖δp_ref‖₂ + ‖V_d⁻¹‖₂ (‖g_p‖₁ + Σ_o ‖|W_o|ᵀ|dc_c|‖₁))
  residual  |info[1] - ρ_true|, ρ_true = ‖b - S dc‖₂ / ‖b‖₂ in 50 digits:
            u_r = eps ‖ |U_d||dc| + Σ|W||V_d⁻¹||W|ᵀ|dc| + |b| ‖₂ / ‖b‖₂
  model     info[2], info[3] against the 50-digit terms of the same δ: eps Σ|term| of each sum
  direct    small cases run at tol = 1e-13 (has_direct): max|δ - δ*| / max|δ*| per parameter
            class (r, t, f, k1, X), δ* the 50-digit dense solve.  Its one K over all runs is set
            by benign at λ = 1e-14 (0.229: S is singular but for the damping), so at every other
            run, where the oracle sits between 1e-7 and 1e-16, this check only excludes a wrong
            solution (+g_p misses it by 1.22 against 0.916), not a loss of digits; the residual
            and back-substitution units carry the precision there
  first     the fallback cases after one iteration, per camera, 2-norm, against x_1 = α M b in 50
            digits (SolveRef.first_iterate): eps (κ₂(S_cc) + c_α) ‖x_1c‖₂; K = 4 x max(oracle, 1)
K of a unit = 4 x the worst ratio of oracle/ba_lm.py (schur_pcg, back_substitute, model_terms) over
all runs (the residual unit: 4 x max(worst, 1)); ORACLE_RATIO holds the measured ratios per run.

Measured (test_ba_solve_hp_cpu.py prints them), the CPU oracle's worst ratio:
  backsub 0.138 (benign at λ = 1e12; 0.03-0.13 elsewhere, 0.092 at κ₂(V_d) = 2.5e15), residual
  0.757 (benign at λ = 1e4, two iterations; below 0.3 elsewhere), model terms 2.19 (δᵀJᵀJδ of
  clamp), direct 0.229 (benign at λ = 1e-14; 5.6e-7 at 1e-8, 8e-9 fewview at 1e-8, 7e-8 narrow,
  below 3e-10 elsewhere); hence K = 0.552, 4, 8.76, 0.916.
  SPD margins (smallest Cholesky pivot / largest diagonal of S_cc, in units of 1e3 eps): S2a 4.0,
  fewview_px 440, clamp 870, narrow 1.9e3, S2b 2.1e3, fewview at 1e-8 2.7e3, S1 5.8e3, every other run above 7e3.
  single at λ = 1e-10: the oracle's CG breaks down at iteration 38 (MAY_BREAK).
  The eight mutations of hp_ref.solve_f64: no clamp 1.5e9 x K (residual, clamp); W's layout
  2.3e16 x K (residual, benign); a dropped observation 3e12 x K, a stale dp 5e13 x K, +g_p 8e14
  x K (backsub); undamped U in S p 3e9 x K (residual); info[1] = 0 on a breakdown 1.1e15 x K;
  a skipped z = M r stays inside K in every unit (0.62 x K at worst: the recurrence residual
  stays true) and is caught by the breakdown it causes (info[4] = 2) and by the iteration count
  (24 for the oracle's 69), not by a unit.
  First iterate of the fallback cases: 0.275 and 1.98 units (ORACLE_FIRST), K_FIRST = 7.96.
Measured on an MI355X (test_gpu_ba_solve_hp.py prints them per run, unit and mode), the kernel's
worst ratio over the implicit, chunked (8, 3) and explicit forms:
  backsub 0.179 (single at 1e-10, 8 chunks; 0.15-0.18 per mode), residual 0.358 (benign),
  model terms 0.983 (gᵀδ, benign), direct 0.229 (benign at λ = 1e-14, every mode; gn 7.5e-15,
  fewview 3.5e-8, single 4.9e-10, narrow 1.2e-7, clamp 1.3e-13, fewview_px 2.7e-12,
  fallback_obs 5.5e-12); first iterate 0.31 (fallback) and 1.92 (fallback_obs).  The adjugate
  V_d⁻¹ sits where numpy's inverse does, κ₂(V_d) = 2.5e15 included.  single at λ = 1e-10 breaks down on the GPU
  too (iteration 39 to 80 by mode) and reports it: info[1] = rho_true = 4e-4 to 1.4e-3.
What check (c) is there for: a solver that zeroes r·r to stop on a breakdown reports info[1] = 0
on the breakdown cases and on single at λ = 1e-10 (real geometry), at rho_true = 1 and 1e-3.
"""
from __future__ import annotations

import functools
import typing

import numpy as np

import ba_edge_cases as E
import ba_lm as L
import hp_ref
import oracle as O

EPS = hp_ref.EPS
SMALL_TOL, SMALL_CAP = 1e-13, 500
SHAPE_TOL, SHAPE_CAP = 1e-12, 300
SHAPE_LAMBDAS = (1e-3, 1e-2, 1e-1)
BENIGN_LAMBDAS = (1e-14, 1e-8, 1e-4, 1.0, 1e4, 1e12)
FALLBACK_LAMBDA = 0.25
FLAG_FALLBACK, FLAG_BREAKDOWN = L.FLAG_FALLBACK, L.FLAG_BREAKDOWN
SPD_MARGIN = 1e3 * EPS                     # Cholesky pivots of every S_cc above this x max diag
MODES = ("implicit", "chunks8", "chunks3", "explicit8")


def _blocks(prob):
    o = O.ba_jtj(prob["cams"], prob["pp"], prob["pts"], prob["cam_idx"], prob["pt_idx"], prob["uv"])
    return {k: np.array(o[k], np.float64) for k in ("U", "V", "W", "gc", "gp")}


def _views(b, rng, cs, n_pt, n_view, tag="benign"):
    ps = []
    for _ in range(n_pt):
        p = b.pt(rng.uniform(-1, 1, size=3))
        for c in rng.choice(len(cs), size=n_view, replace=False):
            b.see(cs[c], p, tag, 0.0)
        ps.append(p)
    return ps


def _benign(seed=31):
    rng = np.random.default_rng(seed)
    b = E._Builder(rng)
    cs = [b.cam(E._benign_cam(rng)) for _ in range(8)]
    _views(b, rng, cs, 60, 4)
    return b.problem()


def _unit_cam(rng):
    """A camera in normalised image units (f ~ 1) 2.5 in front of the unit box: its eight diagonal
    entries of U are within three decades of each other for a point at |p| >= 0.35 (rotation ~1,
    translation ~0.2, f ~|p|^2, k1 ~|p|^6), so a camera of one observation damped by λ = 1e-8
    keeps Cholesky pivots ~1e-8 x 2e-3 of its largest diagonal: the margin SPD_MARGIN asks for.
    (At f ~ 1000 px the same camera has diagonals from 0.04 to 1e7 and no such margin.)"""
    cam = np.zeros(8)
    cam[:3] = rng.uniform(0.05, 0.2) * E._unit(rng)
    cam[3:6] = (rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(2.4, 2.6))
    cam[6] = rng.uniform(0.95, 1.05)
    cam[7] = rng.uniform(-0.02, 0.02)
    return cam


def _fewview_px(seed=32):
    """Pixel units (f ~ 1000), cameras 8..11 of 1, 2, 3, 4 observations: has the SPD margin at
    λ = 1e-4 (440 x), not at 1e-8 (0.04 x)."""
    rng = np.random.default_rng(seed)
    b = E._Builder(rng)
    cs = [b.cam(E._benign_cam(rng)) for _ in range(8)]
    ps = _views(b, rng, cs, 60, 4)
    for n in (1, 2, 3, 4):
        c = b.cam(E._benign_cam(rng))
        for p in rng.choice(ps, size=n, replace=False):
            b.see(c, int(p), "fewview", n)
    return b.problem()


def _fewview(seed=32):
    """Normalised image units throughout (_unit_cam); residuals of 5e-4 (0.5 px at f = 1000)."""
    rng = np.random.default_rng(seed)
    b = E._Builder(rng)
    cs = [b.cam(_unit_cam(rng)) for _ in range(8)]
    ps = []
    for _ in range(60):
        p = b.pt(rng.uniform(-1, 1, size=3))
        for c in rng.choice(8, size=4, replace=False):
            b.see(cs[c], p, "benign", 0.0, residual=5e-4)
        ps.append(p)
    for n in (1, 2, 3, 4):                       # cameras 8..11 hold n observations, |p| >= 0.35
        cam = _unit_cam(rng)
        c = b.cam(cam)
        far = [p for p in ps if np.linalg.norm(
            (E._project(cam, np.zeros(2), b.pts[p])) / cam[6]) >= 0.35]
        for p in rng.choice(far, size=n, replace=False):
            b.see(c, int(p), "fewview", n, residual=5e-4)
    return b.problem()


def _single(seed=33):
    rng = np.random.default_rng(seed)
    b = E._Builder(rng)
    cs = [b.cam(E._benign_cam(rng)) for _ in range(8)]
    _views(b, rng, cs, 50, 4)
    for i in range(12):                          # one observation each
        b.see(cs[i % 8], b.pt(rng.uniform(-1, 1, size=3)), "single", 1)
    p = b.pt(rng.uniform(-1, 1, size=3))         # seen twice by camera 3
    for c in (3, 3, 5):
        b.see(cs[c], p, "duplicate", 2)
    return b.problem()


def _narrow(seed=34):
    """Cameras 8 and 9 are camera 0 with its centre moved by 8 tan(0.05 deg) and 8 tan(0.5 deg)
    across the viewing direction: a point at depth ~8 seen by 0 and 8 (0 and 9) alone has rays
    0.05 (0.5) degrees apart."""
    rng = np.random.default_rng(seed)
    b = E._Builder(rng)
    cs = [b.cam(E._benign_cam(rng)) for _ in range(8)]
    for deg in (0.05, 0.5):
        cam = b.cams[0].copy()
        cam[3] += 8.0 * np.tan(np.radians(deg))  # t = -R C: a shift of t is a shift of the centre
        cs.append(b.cam(cam))
    for _ in range(50):                          # every camera well determined by normal points
        p = b.pt(rng.uniform(-1, 1, size=3))
        for c in rng.choice(10, size=4, replace=False):
            b.see(cs[c], p, "benign", 0.0)
    for other, deg in ((8, 0.05), (9, 0.5)):
        for _ in range(6):
            p = b.at(0, np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 8.0]))
            b.see(cs[0], p, "narrow", deg)
            b.see(cs[other], p, "narrow", deg)
    return b.problem()


def _clamp(seed=35):
    rng = np.random.default_rng(seed)
    b = E._Builder(rng)
    b.pt(rng.uniform(-1, 1, size=3))                                   # unobserved, first
    cs = [b.cam(E._benign_cam(rng)) for _ in range(8)]
    ps = _views(b, rng, cs[:8], 30, 4)
    b.pt(rng.uniform(-1, 1, size=3))                                   # unobserved, middle
    ps += _views(b, rng, cs[:8], 30, 4)
    cam = E._benign_cam(rng)
    cam[6], cam[7] = 200.0, 0.01
    c = b.cam(cam)                                                     # camera 8: the clamp
    for z in (7.0, 7.6, 8.3, 9.0):
        off = rng.uniform(-0.4, 0.4, size=2) / 200.0                   # within 0.4 px, noise none
        p = b.at(c, z * np.array([off[0], off[1], 1.0]))
        b.see(c, p, "clamp", 0.0, residual=0.3)
        for k in rng.choice(8, size=3, replace=False):
            b.see(cs[k], p, "clamp", 0.0)
    b.cam(E._benign_cam(rng))                                          # camera 9: unobserved
    b.pt(rng.uniform(-1, 1, size=3))                                   # unobserved, last
    return b.problem()


S3_COUNTS = (255, 256, 257, 513)
S3_TRACKS = (7, 8, 9, 31, 32, 33, 128, 129)
S3_NCAM, S3_NPT = 33, 583


def _s3(seed=36):
    """Track lengths: the eight of S3_TRACKS spread among tracks of 3 and 4, the 129-track last;
    cameras 0..3 hold S3_COUNTS, the other 29 share the rest evenly.  A track longer than 33 takes
    the cameras in rounds (each round distinct cameras, those with the most left first)."""
    rng = np.random.default_rng(seed)
    n_fill = S3_NPT - len(S3_TRACKS)
    fill = rng.integers(3, 5, size=n_fill).tolist()
    lengths = fill[:]
    for i, t in enumerate(S3_TRACKS[:-1]):
        lengths.insert(10 + 70 * i, t)
    lengths.append(S3_TRACKS[-1])
    n_obs = sum(lengths)
    rest = n_obs - sum(S3_COUNTS)
    counts = list(S3_COUNTS) + [rest // 29 + (1 if i < rest % 29 else 0) for i in range(29)]
    left = np.array(counts, np.int64)
    tracks = [None] * len(lengths)
    for t in sorted(range(len(lengths)), key=lambda i: -lengths[i]):
        need, cams_t = lengths[t], []
        while need:
            order = np.lexsort((rng.random(S3_NCAM), -left))
            pick = [c for c in order[:need] if left[c] > 0]
            assert pick, "S3: track lengths do not fit the camera counts"
            left[pick] -= 1
            cams_t += pick
            need -= len(pick)
        tracks[t] = rng.permutation(cams_t).tolist()
    assert not left.any()
    cams = np.array([E._benign_cam(rng) for _ in range(S3_NCAM)])
    pp = np.tile(E.PP, (S3_NCAM, 1)) + rng.uniform(-5, 5, size=(S3_NCAM, 2))
    pts = rng.uniform(-1, 1, size=(len(lengths), 3))
    ci, pi, uv = [], [], []
    for p, cs in enumerate(tracks):
        for c in cs:
            ci.append(c)
            pi.append(p)
            uv.append(E._project(cams[c], pp[c], pts[p]) + rng.normal(0.0, 0.5, size=2))
    return dict(cams=cams, pp=pp, pts=pts, cam_idx=np.array(ci, np.int32),
                pt_idx=np.array(pi, np.int32), uv=np.array(uv))


def _handmade(breakdown):
    """5 cameras, no points, integer blocks (every product below is exact in float64)."""
    rng = np.random.default_rng(37)
    U = np.zeros((5, 8, 8))
    for c in range(5):
        A = rng.integers(-1, 2, size=(8, 8)).astype(np.float64)
        U[c] = A @ A.T + 8.0 * np.eye(8)                  # SPD, not diagonal
    U[2, 7, :] = 0.0
    U[2, :, 7] = 0.0
    U[2, 7, 7] = -1.0
    gc = rng.integers(-4, 5, size=(5, 8)).astype(np.float64)
    gc[gc == 0] = 1.0
    gc[2, 7] = 3.0 if breakdown else 0.0
    return dict(U=U, V=np.zeros((0, 3, 3)), W=np.zeros((0, 8, 3)), gc=gc, gp=np.zeros((0, 3)))


_PROBLEMS = dict(fallback_obs=_benign, breakdown_obs=_benign, benign=_benign, gn=_benign,
                 fewview=_fewview, fewview_px=_fewview_px, single=_single, narrow=_narrow,
                 clamp=_clamp, zero=_benign, S3=_s3)
SHAPE_CASES = ("S1", "S2a", "S2b", "S3")
HANDMADE = ("fallback", "breakdown")
NEGATIVE_OBS = ("fallback_obs", "breakdown_obs")
NOT_SPD = HANDMADE + NEGATIVE_OBS


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: raw (the blocks before fix_params), blocks (after; the solve's exact inputs), fixed
    ([n_cam, 8] bool or None), cam_idx, pt_idx, n_cam, n_pt, n_obs, prob (the geometry or None)."""
    fixed = None
    if name in HANDMADE:
        prob, raw = None, _handmade(name == "breakdown")
        ci = pi = np.zeros(0, np.int32)
    else:
        prob = E.case(name) if name in ("S1", "S2a", "S2b") else _PROBLEMS[name]()
        raw = _blocks(prob)
        ci, pi = np.array(prob["cam_idx"], np.int32), np.array(prob["pt_idx"], np.int32)
        if name == "zero":
            raw["gc"][:], raw["gp"][:] = 0.0, 0.0
        if name in NEGATIVE_OBS:
            raw["U"][7, 7, :], raw["U"][7, :, 7] = 0.0, 0.0
            raw["U"][7, 7, 7] = -1.0
            raw["W"][ci == 7, 7, :] = 0.0
            raw["gc"][7, 7] = 3.0 if name == "breakdown_obs" else 0.0
        if name == "gn":
            import reconstruction as R
            fixed = np.asarray(R.gauge_mask(prob["cams"], ref=0, fix_intrinsics=True), bool)
    blocks = {k: v.copy() for k, v in raw.items()}
    if fixed is not None:
        L.fix_params(blocks, ci, fixed)
    for d in (raw, blocks):
        for v in d.values():
            v.setflags(write=False)
    return dict(raw=raw, blocks=blocks, fixed=fixed, cam_idx=ci, pt_idx=pi, n_cam=len(raw["U"]),
                n_pt=len(raw["V"]), n_obs=len(ci), prob=prob)


# the chosen λ of the shape cases (test_ba_solve_hp_cpu.py recomputes them): the oracle converges
# at every λ tried (S1 39 / 32 / 20 iterations at 1e-3 / 1e-2 / 1e-1, S2a and S2b 87 / 65 / 34,
# S3 66 / 54 / 32); S2a's one-observation cameras have 0.41 x the SPD margin at 1e-3, 4.0 x at 1e-2
SHAPE_LAMBDA = dict(S1=1e-3, S2a=1e-2, S2b=1e-3, S3=1e-3)


class Run(typing.NamedTuple):
    name: str
    lam: float
    tol: float
    max_iter: int
    tag: str

    @property
    def id(self):
        return f"{self.name}@{self.lam:g}" + (f"/{self.tag}" if self.tag else "")

    @property
    def small(self):
        return self.name not in SHAPE_CASES


def _run(name, lam, tol=SMALL_TOL, cap=SMALL_CAP, tag=""):
    return Run(name, float(lam), float(tol), int(cap), tag)


RUNS = tuple(
    [_run("benign", l) for l in BENIGN_LAMBDAS]
    + [_run("benign", 1e-4, tol=0.1, tag="tol0.1"), _run("benign", 1e-4, cap=3, tag="cap3"),
       _run("gn", 0.0), _run("fewview_px", 1e-4), _run("fewview", 1e-4), _run("fewview", 1e-8), _run("single", 1e-4),
       _run("single", 1e-10), _run("narrow", 1e-6), _run("clamp", 1.0), _run("zero", 1e-4),
       _run("fallback", FALLBACK_LAMBDA), _run("fallback", FALLBACK_LAMBDA, cap=1, tag="cap1"),
       _run("breakdown", FALLBACK_LAMBDA), _run("fallback_obs", 1e-4),
       _run("fallback_obs", 1e-4, cap=1, tag="cap1"), _run("breakdown_obs", 1e-4)]
    + [_run(n, SHAPE_LAMBDA[n], tol=SHAPE_TOL, cap=SHAPE_CAP) for n in SHAPE_CASES])
# the benign runs whose CG is well conditioned: the iteration count is held to the oracle's +- 3
COUNTED = tuple(r for r in RUNS if r.name == "benign" and r.lam >= 1e-4 and r.tag != "cap3")
# single@1e-10: κ₂(V_d) of the single-view points is 2.5e15, one rounding of S p is 1e-4 of |b|
# (u_r) and exceeds the smallest curvature: the oracle's own float64 CG breaks down at iteration
# 38 with rho_true 0.0125.  There, and only there, a breakdown is neither demanded nor forbidden;
# what is demanded is that it is reported honestly (checks c, d, e).
MAY_BREAK = tuple(r for r in RUNS if r.name == "single" and r.lam == 1e-10)
UNITS = ("backsub", "residual", "gd", "q", "direct")

# worst ratio of oracle/ba_lm.py per run and unit, measured (test_ba_solve_hp_cpu.py prints them)
ORACLE_RATIO = {
    "benign@1e-14": dict(backsub=0.0486, residual=0.00197, gd=0.0, q=0.0668, direct=0.229),
    "benign@1e-08": dict(backsub=0.0725, residual=0.00314, gd=0.0, q=0.276, direct=5.59e-07),
    "benign@0.0001": dict(backsub=0.0801, residual=0.079, gd=0.521, q=0.213, direct=4.11e-13),
    "benign@1": dict(backsub=0.0629, residual=0.0893, gd=0.0, q=0.0, direct=3.63e-14),
    "benign@10000": dict(backsub=0.0991, residual=0.757, gd=0.0, q=0.0, direct=7.02e-16),
    "benign@1e+12": dict(backsub=0.138, residual=0.124, gd=0.0, q=1.46, direct=4.19e-16),
    "benign@0.0001/tol0.1": dict(backsub=0.0818, residual=0.0035, gd=0.0, q=0.0189),
    "benign@0.0001/cap3": dict(backsub=0.0469, residual=0.0071, gd=0.545, q=0.0154),
    "gn@0": dict(backsub=0.106, residual=0.00437, gd=0.84, q=1.93, direct=6.63e-15),
    "fewview_px@0.0001": dict(backsub=0.0335, residual=0.00518, gd=0.214, q=0.197, direct=2.18e-12),
    "fewview@0.0001": dict(backsub=0.0821, residual=0.0012, gd=0.0, q=0.0352, direct=2.7e-12),
    "fewview@1e-08": dict(backsub=0.125, residual=0.00897, gd=0.162, q=0.113, direct=8.15e-09),
    "single@0.0001": dict(backsub=0.0572, residual=0.0314, gd=0.0, q=0.463, direct=1.96e-10),
    "single@1e-10": dict(backsub=0.0923, residual=0.0014, gd=0.0162, q=0.0546),
    "narrow@1e-06": dict(backsub=0.0373, residual=0.0104, gd=0.0467, q=0.353, direct=6.87e-08),
    "clamp@1": dict(backsub=0.071, residual=0.0687, gd=0.0, q=2.19, direct=1.26e-13),
    "zero@0.0001": dict(backsub=0.0, residual=0.0, gd=0.0, q=0.0, direct=0.0),
    "fallback@0.25": dict(backsub=0.0, residual=0.279, gd=0.907, q=0.0, direct=2.21e-16),
    "fallback@0.25/cap1": dict(backsub=0.0, residual=0.0496, gd=0.0, q=0.343),
    "breakdown@0.25": dict(backsub=0.0, residual=0.0, gd=0.0, q=0.0),
    "fallback_obs@0.0001": dict(backsub=0.0719, residual=0.00989, gd=0.0, q=0.196, direct=3e-13),
    "fallback_obs@0.0001/cap1": dict(backsub=0.0685, residual=0.00623, gd=0.635, q=0.118),
    "breakdown_obs@0.0001": dict(backsub=0.105, residual=0.0, gd=0.562, q=0.839),
    "S1@0.001": dict(backsub=0.0875, residual=0.00367, gd=0.0, q=1.1),
    "S2a@0.01": dict(backsub=0.129, residual=0.0126, gd=0.58, q=0.749),
    "S2b@0.001": dict(backsub=0.131, residual=7.51e-05, gd=0.0, q=0.156),
    "S3@0.001": dict(backsub=0.0901, residual=0.000583, gd=0.0, q=0.279),
}


def _worst(*units):
    return max((r.get(u, 0.0) for r in ORACLE_RATIO.values() for u in units), default=0.0)


# backsub 4 x 0.138 = 0.552; residual 4 x max(0.757, 1) = 4; the two model terms share one K,
# 4 x 2.19 = 8.76; direct 4 x 0.229 = 0.916 (benign at λ = 1e-14: S is singular but for the damping)
K = dict(backsub=4.0 * _worst("backsub"), residual=4.0 * max(_worst("residual"), 1.0),
         gd=4.0 * _worst("gd", "q"), q=4.0 * _worst("gd", "q"), direct=4.0 * _worst("direct"))


def run_id(r):
    return r.id


def solve_args(run):
    c = case(run.name)
    b = c["blocks"]
    return (b["U"], b["V"], b["W"], b["gc"], b["gp"], c["cam_idx"], c["pt_idx"], run.lam)


@functools.lru_cache(maxsize=None)
def _reference(name, lam):
    return hp_ref.solve_blocks(*solve_args(_run(name, lam)))


def reference(run):
    """The 50-digit SolveRef of a run's blocks and λ (cached per process)."""
    return _reference(run.name, run.lam)


@functools.lru_cache(maxsize=None)
def oracle(run):
    """(dc, dp, info [5]) of oracle/ba_lm.py on the run, info as sfm_ba_solve's."""
    a = solve_args(run)
    dc, dp, it, rel, flag = L.schur_pcg(*a, max_iter=run.max_iter, tol=run.tol, flags=True)
    gd, q = L.model_terms(*a[:7], dc, dp)
    return dc, dp, np.array([it, rel, gd, q, flag], np.float64)


def spd_margin(run):
    """min over cameras of (smallest Cholesky pivot of S_cc) / (largest diagonal entry of S_cc),
    float64, the oracle's S_cc."""
    _, _, _, S, _ = L.schur_rhs_and_precond(*solve_args(run))
    piv = L.cholesky_pivots(S)
    return float((piv.min(1) / np.diagonal(S, axis1=1, axis2=2).max(1)).min())


# the fallback cases stopped after one iteration: dc = x_1 = α M b shows the preconditioner
FIRST_RUNS = tuple(r for r in RUNS if r.tag == "cap1")
# the oracle's measured ratios (fallback_obs: the unit leaves out the rounding of S_cc and b
# themselves, which the diagonal form of camera 7 passes on undamped)
ORACLE_FIRST = {"fallback@0.25/cap1": 0.276, "fallback_obs@0.0001/cap1": 1.99}
K_FIRST = 4.0 * max(max(ORACLE_FIRST.values()), 1.0)


@functools.lru_cache(maxsize=None)
def _first(name, lam):
    return reference(_run(name, lam)).first_iterate()


def first_ratio(run, dc):
    """(worst ‖dc_c - x_1c‖₂ / unit_c over the cameras, the 50-digit fallback mask)."""
    x1, bad, unit = _first(run.name, run.lam)
    dc = np.asarray(dc, np.float64).reshape(x1.shape)
    err = np.where(np.isfinite(dc).all(1), np.linalg.norm(dc - x1, axis=1), np.inf)
    return _ratio(err, unit), bad


def _ratio(err, unit):
    err, unit = np.asarray(err, np.float64), np.asarray(unit, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(unit > 0, err / unit, np.where(err == 0, 0.0, np.inf))
    q = np.where(np.isfinite(err), q, np.inf)
    return float(q.max()) if q.size else 0.0


def has_direct(run):
    """Check (g) applies: a small case run at tol 1e-13 to the cap of 500, whatever the solve
    under test reports.  Not the breakdown cases (δ = 0 by construction) and not MAY_BREAK,
    where the oracle itself does not reach tol."""
    return run.small and run.tol == SMALL_TOL and run.max_iter == SMALL_CAP \
        and not run.name.startswith("breakdown") and run not in MAY_BREAK


def measure(run, dc, dp, info, direct=None):
    """Ratios of one solve's (dc, dp, info) against the reference, per unit, and rho_true, u_r.
    direct (default: has_direct(run)): also against δ*."""
    ref = reference(run)
    dc = np.asarray(dc, np.float64).reshape(ref.nc, 8)
    dp = np.asarray(dp, np.float64).reshape(ref.npt, 3)
    info = np.asarray(info, np.float64)
    out = {}
    if not np.all(np.isfinite(dc)):
        return dict(backsub=np.inf, residual=np.inf, gd=np.inf, q=np.inf, direct=np.inf,
                    rho_true=np.inf, u_r=0.0)
    err, nrm = ref.backsub_error(dc, dp)
    out["backsub"] = _ratio(err, ref.unit_backsub(dc, nrm))
    rho, ur = ref.solve_residual(dc), ref.unit_residual(dc)
    out["rho_true"], out["u_r"] = rho, ur
    out["residual"] = _ratio(abs(info[1] - rho), ur)
    if np.all(np.isfinite(dp)):
        (gd, q), (ugd, uq) = ref.model_terms(dc, dp), ref.unit_model(dc, dp)
        out["gd"], out["q"] = _ratio(abs(info[2] - gd), ugd), _ratio(abs(info[3] - q), uq)
    else:
        out["gd"] = out["q"] = np.inf
    if has_direct(run) if direct is None else direct:
        out["direct"] = max(ref.direct_error(dc, dp).values())
    return out


def failures(run, dc, dp, info, m, k=None, oracle_iters=None):
    """The checks (a)-(g) of one solve as a list of messages (empty: all hold); m = measure(...)."""
    k = K if k is None else k
    c, ref = case(run.name), reference(run)
    dc = np.asarray(dc, np.float64).reshape(ref.nc, 8)
    dp = np.asarray(dp, np.float64).reshape(ref.npt, 3)
    info = np.asarray(info, np.float64)
    bad = []
    for u in UNITS:                                                        # (a) (c) (f) (g)
        if u not in m and (u != "direct" or has_direct(run)):
            bad.append(f"{u}: not measured")
        if u in m and not m[u] <= k[u]:
            bad.append(f"{u}: {m[u]:.3g} > K = {k[u]:.3g}")
    if not np.all(np.isfinite(info)):
        bad.append(f"info not finite: {info}")
    if np.any(dp[~ref.seen] != 0.0):                                       # (b)
        bad.append("dp != 0 for an unobserved point")
    seen_cam = np.bincount(c["cam_idx"], minlength=ref.nc) > 0
    if c["prob"] is not None and np.any(dc[~seen_cam] != 0.0):
        bad.append("dc != 0 for an unobserved camera")
    if c["fixed"] is not None and np.any(dc[c["fixed"]] != 0.0):
        bad.append("dc != 0 for a held parameter")
    it, flag = int(info[0]), int(info[4])
    broke = bool(flag & FLAG_BREAKDOWN)
    if it < run.max_iter and not broke and not m["rho_true"] <= run.tol + k["residual"] * m["u_r"]:
        bad.append(f"stopped at {it} < {run.max_iter} with rho_true {m['rho_true']:.3g} > tol")  # (d)
    if it > run.max_iter or (info[1] > run.tol and not broke and it != run.max_iter):            # (e)
        bad.append(f"iterations {it}, cap {run.max_iter}, info[1] {info[1]:.3g}")
    want = dict(fallback=FLAG_FALLBACK, breakdown=FLAG_FALLBACK | FLAG_BREAKDOWN,
                fallback_obs=FLAG_FALLBACK, breakdown_obs=FLAG_FALLBACK | FLAG_BREAKDOWN
                ).get(run.name, 0)
    if (flag | FLAG_BREAKDOWN if run in MAY_BREAK else flag) != (want | FLAG_BREAKDOWN
                                                                 if run in MAY_BREAK else want):
        bad.append(f"info[4] = {flag}, expected {want}")
    if run.name == "zero" and (it != 0 or info[1] != 0.0 or np.any(dc != 0) or np.any(dp != 0)):
        bad.append("zero gradient: an iteration, a residual or a step")
    if run.tag == "cap3" and not (it == 3 and info[1] > run.tol):
        bad.append(f"cap 3: iterations {it}, info[1] {info[1]:.3g}")
    if run.name.startswith("breakdown") and not (it == 1 and np.all(dc == 0.0) and info[1] == 1.0):
        bad.append(f"breakdown at iteration 0: iterations {it}, info[1] {info[1]:.3g}")
    if oracle_iters is not None and run in COUNTED and abs(it - oracle_iters) > 3:
        bad.append(f"iterations {it}, the oracle's {oracle_iters}")
    return bad


def check(run, dc, dp, info, label, k=None, oracle_iters=None):
    """Prints the ratios of one solve and asserts the checks (a)-(g)."""
    k = K if k is None else k
    m = measure(run, dc, dp, info)
    print(f"{run.id} {label}: " + " ".join(f"{u}={m[u]:.3g}" for u in UNITS if u in m)
          + f"  rho_true={m['rho_true']:.3g} info={np.asarray(info).tolist()}")
    bad = failures(run, dc, dp, info, m, k, oracle_iters)
    assert not bad, f"{run.id} {label}: " + "; ".join(bad)
    return m
