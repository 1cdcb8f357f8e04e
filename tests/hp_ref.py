"""50-digit references for the steps after the match graph (test infrastructure, mpmath).

Written from the specs in the kernel headers (csrc/camera_model.h, csrc/triangulate.hip,
csrc/ba.hip, csrc/two_view_pose.hip), not from the kernels: every quantity is formed in 50-digit arithmetic from the
float64 inputs, so the only error a comparison charges to the code under test is its own.

  rotmat(r)                                   Rodrigues; the spec's first-order form for |r|^2 <= 1e-20
  rot_err(r_out, R_ref)                       max |rotmat(r_out) - R_ref|
  exp_so3(axis, theta)                        exp(theta [a]x) for a unit axis given in 50 digits
  triangulate(cams, pp, pt_ptr, cam_idx, uv)  multi-view DLT, statistics, status, eigenvalues
  stats_f64(...)                              the three statistics at a given X, float64 (for
                                              propagating a point tolerance to the statistics)
  ba_obs(cam, pp, X, uv, loss_s)              one BA observation: residual, 2x11 Jacobian by central
                                              differences in 50 digits, Cauchy w and rho
  ba_assemble(...)                            the whole linearisation summed in 50 digits, with units
  ba_residuals(...)                           residuals, rho and the cost alone (large problems)
  ba_f64(...), ba_units(...)                  float64 restatement of the linearisation carrying a
                                              first-order error unit for every entry
  solve_blocks(U, V, W, gc, gp, ci, pi, lam)  the BA step solve (csrc/ba_solve.hip) on the float64
                                              blocks: a SolveRef with V_d^-1, its condition, b, the
                                              implicit S x, solve_residual, solve_backsub,
                                              solve_direct, model_terms and the units of each
  solve_f64(...)                              float64 restatement of the solve with a mut switch
  undistort_exact(xd, k1)                     the true inverse of the radial distortion, its
                                              contraction factor; undistort_steps: the spec's steps
  pose_normal(x1, x2, mask)                   the essential fit (csrc/two_view_pose.hip): exact N, its
                                              eigenvalues and null vector, the null vector of A
  pose_decompose(E)                           SVD of a float64 E, the four (R, t), status 2
  pose_vote(R, t, x1, x2, mask)               depth numerators and ray-angle keys with their units
  pose_f64(x1, x2, mask, mut)                 float64 restatement of the pose spec with a mut switch
"""
from __future__ import annotations

import functools

import mpmath as mp
import numpy as np

DPS = 50
UNDISTORT_ITERS = 10


def _hp(fn):
    @functools.wraps(fn)
    def wrapped(*a, **k):
        with mp.workdps(DPS):
            return fn(*a, **k)
    return wrapped


def _vec(r):
    return [mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x for x in r]


@_hp
def rotmat(r):
    """3x3 list of mpf: I + sin θ K + (1 - cos θ) K², K = [r/θ]x; I + [r]x for |r|² <= 1e-20 (the
    camera model's own definition there, not an approximation to be refined)."""
    r = _vec(r)
    th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    one, zero = mp.mpf(1), mp.mpf(0)
    if th2 <= mp.mpf("1e-20"):
        return [[one, -r[2], r[1]], [r[2], one, -r[0]], [-r[1], r[0], one]]
    th = mp.sqrt(th2)
    return exp_so3([x / th for x in r], th)


@_hp
def exp_so3(axis, theta):
    """exp(θ [a]x); the axis is normalised in 50 digits first."""
    a = _vec(axis)
    n = mp.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    a = [x / n for x in a]
    theta = mp.mpf(theta)
    s, c = mp.sin(theta), mp.cos(theta)
    C = 1 - c
    K = [[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]
    return [[(c if i == j else 0) + C * a[i] * a[j] + s * K[i][j] for j in range(3)]
            for i in range(3)]


@_hp
def matmul(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)]
            for i in range(3)]


@_hp
def to_f64(R):
    return np.array([[float(x) for x in row] for row in R])


@_hp
def rot_err(r_out, R_ref):
    """max |rotmat(r_out) - R_ref| as a float; r_out float64, R_ref 3x3 of mpf."""
    R = rotmat(r_out)
    return float(max(abs(R[i][j] - R_ref[i][j]) for i in range(3) for j in range(3)))


def _undistort(xd, k1):
    x0, x1 = xd
    for _ in range(UNDISTORT_ITERS):
        s = 1 + k1 * (x0 * x0 + x1 * x1)
        x0, x1 = xd[0] / s, xd[1] / s
    return x0, x1


@_hp
def triangulate(cams, pp, pt_ptr, cam_idx, uv):
    """Spec of csrc/triangulate.hip's header in 50 digits.  Returns a dict of float64 arrays:
    pts [n,3], stats [n,4] (mean reprojection error px, largest ray angle deg, smallest depth,
    status), lam [n,4] (eigenvalues of M, ascending; zero for status 1) and ratio [n]
    (|h3| / |h0..2| of the chosen eigenvector; zero for status 1)."""
    cams = np.asarray(cams, np.float64)
    pp = np.asarray(pp, np.float64)
    uv = np.asarray(uv, np.float64)
    n = len(pt_ptr) - 1
    pts, stats = np.zeros((n, 3)), np.zeros((n, 4))
    lam, ratio = np.zeros((n, 4)), np.zeros(n)
    cam_cache = {}

    def camera(c):
        if c not in cam_cache:
            R = rotmat(cams[c, :3])
            t = _vec(cams[c, 3:6])
            C = [-(R[0][j] * t[0] + R[1][j] * t[1] + R[2][j] * t[2]) for j in range(3)]
            cam_cache[c] = (R, t, C, mp.mpf(float(cams[c, 6])), mp.mpf(float(cams[c, 7])),
                            _vec(pp[c]))
        return cam_cache[c]

    for p in range(n):
        o0, o1 = int(pt_ptr[p]), int(pt_ptr[p + 1])
        if o1 - o0 < 2:
            stats[p, 3] = 1
            continue
        M = mp.zeros(4, 4)
        for o in range(o0, o1):
            R, t, _, f, k1, c_pp = camera(int(cam_idx[o]))
            m = _vec(uv[o])
            x0, x1 = _undistort(((m[0] - c_pp[0]) / f, (m[1] - c_pp[1]) / f), k1)
            P = [R[i] + [t[i]] for i in range(3)]
            for x, i in ((x0, 0), (x1, 1)):
                row = [x * P[2][j] - P[i][j] for j in range(4)]
                for a in range(4):
                    for b in range(4):
                        M[a, b] += row[a] * row[b]
        E, Q = mp.eigsy(M)
        order = sorted(range(4), key=lambda k: E[k])
        lam[p] = [float(E[k]) for k in order]
        h = [Q[i, order[0]] for i in range(4)]
        nh = mp.sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2])
        ratio[p] = float(abs(h[3]) / nh) if nh > 0 else np.inf
        if not abs(h[3]) > mp.mpf("1e-12") * nh:
            stats[p, 3] = 2
            continue
        X = [h[i] / h[3] for i in range(3)]
        pts[p] = [float(x) for x in X]
        err, dmin, rays = mp.mpf(0), None, []
        for o in range(o0, o1):
            R, t, C, f, k1, c_pp = camera(int(cam_idx[o]))
            m = _vec(uv[o])
            Pc = [R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + t[i] for i in range(3)]
            dmin = Pc[2] if dmin is None or Pc[2] < dmin else dmin
            q0, q1 = Pc[0] / Pc[2], Pc[1] / Pc[2]
            d = 1 + k1 * (q0 * q0 + q1 * q1)
            e0, e1 = f * d * q0 + c_pp[0] - m[0], f * d * q1 + c_pp[1] - m[1]
            err += mp.sqrt(e0 * e0 + e1 * e1)
            a = [X[j] - C[j] for j in range(3)]
            na = mp.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
            rays.append([x / na for x in a])
        cmin = mp.mpf(1)
        for i in range(len(rays)):
            a = rays[i]
            for j in range(i + 1, len(rays)):
                b = rays[j]
                cmin = min(cmin, a[0] * b[0] + a[1] * b[1] + a[2] * b[2])
        ang = mp.degrees(mp.acos(max(mp.mpf(-1), min(mp.mpf(1), cmin))))
        stats[p] = (float(err / (o1 - o0)), float(ang), float(dmin), 0 if dmin > 0 else 3)
    return dict(pts=pts, stats=stats, lam=lam, ratio=ratio)


def _rotmat_f64(r):
    return to_f64(rotmat(r))


def stats_f64(cams, pp, cam_idx, uv, X):
    """(mean reprojection error px, largest ray angle deg, smallest depth) of one track at X, in
    float64 with the cameras' rotation matrices rounded from the 50-digit ones.  Only for
    propagating a tolerance on X to the statistics: differences of this function around X_ref."""
    cams = np.asarray(cams, np.float64)
    ci = np.asarray(cam_idx)
    R = np.stack([_cached_R(cams[c, :3]) for c in ci])
    t, f, k1 = cams[ci, 3:6], cams[ci, 6], cams[ci, 7]
    P = np.einsum("oij,j->oi", R, X) + t
    q = P[:, :2] / P[:, 2:]
    d = 1.0 + k1 * (q * q).sum(1)
    e = (f * d)[:, None] * q + np.asarray(pp)[ci] - np.asarray(uv)
    a = np.asarray(X)[None, :] + np.einsum("oji,oj->oi", R, t)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    cmin = min(1.0, (a @ a.T).min())
    return np.array([np.linalg.norm(e, axis=1).mean(), np.degrees(np.arccos(max(-1.0, cmin))),
                     P[:, 2].min()])


@functools.lru_cache(maxsize=None)
def _cached_R_key(key):
    return _rotmat_f64(np.array(key))


def _cached_R(r):
    return _cached_R_key(tuple(float(x) for x in r))


# ---- bundle-adjustment linearisation --------------------------------------------------------------
# Spec (headers of csrc/camera_model.h and csrc/ba.hip): r = f (1 + k1 |p|^2) p + pp - uv,
# p = (P0/P2, P1/P2), P = rotmat(r) X + t; e = |r|^2; Cauchy w = 1 / (1 + e/s^2),
# rho = s^2 log1p(e/s^2) for loss_s > 0, else w = 1, rho = e.  The Jacobian's 11 columns follow the
# increment ba_update_kernel applies: R <- exp([d]x) R (3), then t (3), f, k1 and X (3) additive.

FD_STEP = "1e-17"          # central differences in 50 digits: good to ~30 digits
EPS = float(np.finfo(np.float64).eps)
BA_OUTPUTS = ("res", "W", "U", "V", "gc", "gp", "cost")


@functools.lru_cache(maxsize=None)
def _increments():
    """(h, [exp(+h e_k)], [exp(-h e_k)]): the six rotation increments, formed once."""
    with mp.workdps(DPS):
        h = mp.mpf(FD_STEP)
        ax = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
        return h, [exp_so3(a, h) for a in ax], [exp_so3(a, -h) for a in ax]


def _residual(R, t, f, k1, X, c_pp, m):
    P = [R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + t[i] for i in range(3)]
    p0, p1 = P[0] / P[2], P[1] / P[2]
    d = 1 + k1 * (p0 * p0 + p1 * p1)
    return [f * d * p0 + c_pp[0] - m[0], f * d * p1 + c_pp[1] - m[1]], P


@functools.lru_cache(maxsize=None)
def _ba_obs_geom(key):
    """(residual [2], Jacobian 2x11, P) of one observation in 50 digits; key = the 15 float64
    inputs (cam 8, pp 2, X 3, uv 2).  Cached: the loss does not enter."""
    with mp.workdps(DPS):
        v = [mp.mpf(x) for x in key]
        R, t, f, k1 = rotmat(v[0:3]), v[3:6], v[6], v[7]
        c_pp, X, m = v[8:10], v[10:13], v[13:15]
        h, Ep, Em = _increments()
        r0, P = _residual(R, t, f, k1, X, c_pp, m)
        J = [[None] * 11, [None] * 11]

        def put(col, plus, minus):
            for a in range(2):
                J[a][col] = (plus[a] - minus[a]) / (2 * h)

        def bump(vec, k, s):
            return [x + s * h if i == k else x for i, x in enumerate(vec)]

        for k in range(3):
            put(k, _residual(matmul(Ep[k], R), t, f, k1, X, c_pp, m)[0],
                _residual(matmul(Em[k], R), t, f, k1, X, c_pp, m)[0])
            put(3 + k, _residual(R, bump(t, k, 1), f, k1, X, c_pp, m)[0],
                _residual(R, bump(t, k, -1), f, k1, X, c_pp, m)[0])
            put(8 + k, _residual(R, t, f, k1, bump(X, k, 1), c_pp, m)[0],
                _residual(R, t, f, k1, bump(X, k, -1), c_pp, m)[0])
        put(6, _residual(R, t, f + h, k1, X, c_pp, m)[0], _residual(R, t, f - h, k1, X, c_pp, m)[0])
        put(7, _residual(R, t, f, k1 + h, X, c_pp, m)[0], _residual(R, t, f, k1 - h, X, c_pp, m)[0])
        return r0, J, P


def _obs_key(cam, pp, X, uv):
    return tuple(float(x) for x in (*cam, *pp, *X, *uv))


def _loss_terms(r, loss_s):
    e = r[0] * r[0] + r[1] * r[1]
    if loss_s > 0:
        s2 = mp.mpf(float(loss_s)) ** 2
        return e, 1 / (1 + e / s2), s2 * mp.log1p(e / s2)
    return e, mp.mpf(1), e


@_hp
def ba_obs(cam, pp, X, uv, loss_s=0.0):
    """One observation in 50 digits on the float64 inputs: dict of mpf r [2], J [2][11] (central
    differences of the residual, no analytic formula), P [3], e, w, rho."""
    r, J, P = _ba_obs_geom(_obs_key(cam, pp, X, uv))
    e, w, rho = _loss_terms(r, loss_s)
    return dict(r=r, J=J, P=P, e=e, w=w, rho=rho)


@_hp
def ba_residuals(cams, pp, pts, cam_idx, pt_idx, uv, loss_s=0.0):
    """res [n,2], rho [n] as float64 and cost = sum rho / 2 (summed in 50 digits): the residual
    alone, for problems too large for the finite-difference Jacobian."""
    n = len(cam_idx)
    res, rho, cost = np.zeros((n, 2)), np.zeros(n), mp.mpf(0)
    rot = {}
    for o in range(n):
        c, p = int(cam_idx[o]), int(pt_idx[o])
        if c not in rot:
            rot[c] = rotmat(cams[c, :3])
        cam = _vec(cams[c])
        r, _ = _residual(rot[c], cam[3:6], cam[6], cam[7], _vec(pts[p]), _vec(pp[c]), _vec(uv[o]))
        _, _, rh = _loss_terms(r, loss_s)
        res[o], rho[o] = [float(x) for x in r], float(rh)
        cost += rh / 2
    return res, rho, float(cost)


@_hp
def ba_assemble(cams, pp, pts, cam_idx, pt_idx, uv, loss_s=0.0):
    """The linearisation of a whole problem, every product and sum in 50 digits, returned as
    float64: res [n,2], W [n,8,3] = w Jc^T Jp, U [n_cam,8,8] = sum w Jc^T Jc and gc [n_cam,8] =
    sum w Jc^T r over each camera's observations, V [n_pt,3,3], gp [n_pt,3] over each point's,
    cost = sum rho / 2, J [n,2,11], w [n], rho [n]; and "unit": the tolerance unit of every entry
    of the seven outputs (ba_units)."""
    cams, pp, pts, uv = (np.asarray(a, np.float64) for a in (cams, pp, pts, uv))
    n, nc, npt = len(cam_idx), len(cams), len(pts)
    zero = mp.mpf(0)
    U = [[[zero] * 8 for _ in range(8)] for _ in range(nc)]
    gc = [[zero] * 8 for _ in range(nc)]
    V = [[[zero] * 3 for _ in range(3)] for _ in range(npt)]
    gp = [[zero] * 3 for _ in range(npt)]
    out = dict(res=np.zeros((n, 2)), W=np.zeros((n, 8, 3)), J=np.zeros((n, 2, 11)), w=np.zeros(n),
               rho=np.zeros(n))
    cost = zero
    for o in range(n):
        c, p = int(cam_idx[o]), int(pt_idx[o])
        q = ba_obs(cams[c], pp[c], pts[p], uv[o], loss_s)
        r, J, w = q["r"], q["J"], q["w"]
        Jc = [J[0][:8], J[1][:8]]
        Jp = [J[0][8:], J[1][8:]]
        cost += q["rho"] / 2
        out["res"][o] = [float(x) for x in r]
        out["J"][o] = [[float(x) for x in row] for row in J]
        out["w"][o], out["rho"][o] = float(w), float(q["rho"])
        for i in range(8):
            for j in range(i, 8):
                U[c][i][j] += w * (Jc[0][i] * Jc[0][j] + Jc[1][i] * Jc[1][j])
            gc[c][i] += w * (Jc[0][i] * r[0] + Jc[1][i] * r[1])
            for j in range(3):
                out["W"][o, i, j] = float(w * (Jc[0][i] * Jp[0][j] + Jc[1][i] * Jp[1][j]))
        for i in range(3):
            for j in range(i, 3):
                V[p][i][j] += w * (Jp[0][i] * Jp[0][j] + Jp[1][i] * Jp[1][j])
            gp[p][i] += w * (Jp[0][i] * r[0] + Jp[1][i] * r[1])
    sym = lambda M, k: np.array([[[float(B[min(i, j)][max(i, j)]) for j in range(k)]
                                  for i in range(k)] for B in M]).reshape(len(M), k, k)
    out.update(U=sym(U, 8), V=sym(V, 3), cost=float(cost),
               gc=np.array([[float(x) for x in g] for g in gc]).reshape(nc, 8),
               gp=np.array([[float(x) for x in g] for g in gp]).reshape(npt, 3))
    out["unit"] = ba_units(cams, pp, pts, cam_idx, pt_idx, uv, loss_s)
    return out


# ---- float64 restatement with first-order error units ---------------------------------------------
# Every quantity is a (value, unit) pair of numpy arrays over the observations.  The value is the
# float64 restatement; the unit is the first-order propagation of a relative eps on t, X, f, k1, pp
# and uv and an absolute eps on the entries of R, plus eps |q| per operation:
#   u(a b) = |a| u(b) + |b| u(a) + eps |a b|,   u(sum) = sum u + eps sum |term|.

class VU:
    __slots__ = ("v", "u")

    def __init__(self, v, u=None):
        self.v = np.asarray(v, np.float64)
        self.u = np.zeros_like(self.v) if u is None else np.asarray(u, np.float64)

    @staticmethod
    def rel(x):
        return VU(x, EPS * np.abs(x))

    @staticmethod
    def absolute(x):
        x = np.asarray(x, np.float64)
        return VU(x, np.full_like(x, EPS))

    def __mul__(self, o):
        v = self.v * o.v
        return VU(v, np.abs(self.v) * o.u + np.abs(o.v) * self.u + EPS * np.abs(v))

    def __truediv__(self, o):
        v = self.v / o.v
        return VU(v, self.u / np.abs(o.v) + np.abs(v) * o.u / np.abs(o.v) + EPS * np.abs(v))

    def __neg__(self):
        return VU(-self.v, self.u)

    def scale(self, k):
        """Times a power of two: exact."""
        return VU(self.v * k, self.u * abs(k))


def vsum(terms):
    """Left-to-right float64 sum; unit sum u + eps sum |term|."""
    v, u, a = terms[0].v, terms[0].u, np.abs(terms[0].v)
    for t in terms[1:]:
        v, u, a = v + t.v, u + t.u, a + np.abs(t.v)
    return VU(v, u + EPS * a)


def _log1p(x):
    v = np.log1p(x.v)
    return VU(v, x.u / np.abs(1.0 + x.v) + EPS * np.abs(v))


def rotmat_f64(r, mut=""):
    """[n,3,3] float64 Rodrigues of r [n,3] (numpy), first-order form for |r|^2 <= 1e-20.
    Mutations: "e" first-order form up to 1e-12, "f" sin / cos rounded to float32."""
    r = np.asarray(r, np.float64).reshape(-1, 3)
    th2 = (r * r).sum(1)
    small = th2 <= (1e-12 if mut == "e" else 1e-20)
    th = np.sqrt(np.where(small, 1.0, th2))
    s, c = np.sin(th), np.cos(th)
    if mut == "f":
        s, c = s.astype(np.float32).astype(np.float64), c.astype(np.float32).astype(np.float64)
    a = r / th[:, None]
    K = np.zeros((len(r), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -a[:, 2], a[:, 1], -a[:, 0]
    K -= K.transpose(0, 2, 1)
    full = (c[:, None, None] * np.eye(3) + (1.0 - c)[:, None, None] * a[:, :, None] * a[:, None, :]
            + s[:, None, None] * K)
    K1 = np.zeros_like(K)
    K1[:, 0, 1], K1[:, 0, 2], K1[:, 1, 2] = -r[:, 2], r[:, 1], -r[:, 0]
    K1 -= K1.transpose(0, 2, 1)
    return np.where(small[:, None, None], np.eye(3) + K1, full)


def ba_terms_f64(cams, pp, pts, cam_idx, pt_idx, uv, loss_s=0.0, mut=""):
    """The per-observation quantities of the linearisation as VU pairs (chain rule written from
    the spec): dict of res [2], J [2][11], w, rho, hrho (= rho / 2) and the summands W [8][3],
    U [8][8], gc [8], V [3][3], gp [3].  mut: one of the mutations a-f, h of the mutation check
    (tests/test_ba_hp_cpu.py); never set otherwise."""
    cams, pp, pts, uv = (np.asarray(a, np.float64) for a in (cams, pp, pts, uv))
    ci, pi = np.asarray(cam_idx, np.int64), np.asarray(pt_idx, np.int64)
    Rn = rotmat_f64(cams[:, :3], mut)[ci]
    R = [[VU.absolute(Rn[:, i, j]) for j in range(3)] for i in range(3)]
    X = [VU.rel(pts[pi, j]) for j in range(3)]
    t = [VU.rel(cams[ci, 3 + j]) for j in range(3)]
    f, k1 = VU.rel(cams[ci, 6]), VU.rel(cams[ci, 7])
    c_pp = [VU.rel(pp[ci, a]) for a in range(2)]
    m = [VU.rel(uv[:, a]) for a in range(2)]
    one = VU(np.ones(len(ci)))
    Y = [vsum([R[i][j] * X[j] for j in range(3)]) for i in range(3)]
    P = [vsum([R[i][j] * X[j] for j in range(3)] + [t[i]]) for i in range(3)]
    p = [P[0] / P[2], P[1] / P[2]]
    q = vsum([p[0] * p[0], p[1] * p[1]])
    d = vsum([one, k1 * q])
    fd = f * d
    res = [vsum([fd * p[a], c_pp[a], -m[a]]) for a in range(2)]
    e = vsum([res[0] * res[0], res[1] * res[1]])
    if loss_s > 0:
        s2 = VU.rel(np.full(len(ci), float(loss_s) * float(loss_s)))
        x = e / (VU.rel(np.full(len(ci), float(loss_s))) if mut == "d" else s2)
        w = one / vsum([one, x])
        rho = s2 * (VU(np.log(1.0 + x.v), _log1p(x).u) if mut == "h" else _log1p(x))
    else:
        w, rho = one, e
    # M = d pred / d p, D = d p / d P, A = M D
    cross = (k1 * p[0] * p[1]).scale(1.0 if mut == "a" else 2.0)
    M = [[f * vsum([d, (k1 * p[0] * p[0]).scale(2.0)]), f * cross],
         [f * cross, f * vsum([d, (k1 * p[1] * p[1]).scale(2.0)])]]
    iz = one / P[2]
    A = [[M[a][0] * iz, M[a][1] * iz, -(vsum([M[a][0] * p[0], M[a][1] * p[1]]) * iz)]
         for a in range(2)]
    # d P / d delta = -[Y]x: column j is e_j x Y
    sgn = -1.0 if mut == "b" else 1.0
    J = [[vsum([-(A[a][1] * Y[2]), A[a][2] * Y[1]]),
          vsum([(A[a][0] * Y[2]).scale(sgn), -(A[a][2] * Y[0])]),
          vsum([-(A[a][0] * Y[1]), A[a][1] * Y[0]]),
          A[a][0], A[a][1], A[a][2],
          d * p[a], (q * p[a]) if mut == "c" else (f * q * p[a])]
         + [vsum([A[a][k] * R[k][j] for k in range(3)]) for j in range(3)] for a in range(2)]
    Jc, Jp = [J[0][:8], J[1][:8]], [J[0][8:], J[1][8:]]
    jtj = lambda Ja, i, Jb, j: w * vsum([Ja[0][i] * Jb[0][j], Ja[1][i] * Jb[1][j]])
    jtr = lambda Ja, i: w * vsum([Ja[0][i] * res[0], Ja[1][i] * res[1]])
    return dict(res=res, J=J, w=w, rho=rho, hrho=rho.scale(0.5),
                W=[[jtj(Jc, i, Jp, j) for j in range(3)] for i in range(8)],
                U=[[jtj(Jc, min(i, j), Jc, max(i, j)) for j in range(8)] for i in range(8)],
                gc=[jtr(Jc, i) for i in range(8)],
                V=[[jtj(Jp, min(i, j), Jp, max(i, j)) for j in range(3)] for i in range(3)],
                gp=[jtr(Jp, i) for i in range(3)])


def _stack(x, field):
    """Nested lists of VU -> array [n, ...] of the values or the units."""
    if isinstance(x, VU):
        return getattr(x, field)
    return np.stack([_stack(y, field) for y in x], axis=-1) if isinstance(x[0], VU) else \
        np.stack([_stack(y, field) for y in x], axis=-2)


def _segment(terms, index, n, exact=False, drop=None):
    """Sums of the summands `terms` (nested VU) over equal `index`: (values [n, ...], units).
    Values: numpy's sequential sum, or math.fsum of the float64 summands (exact=True).
    drop: an observation left out of the value (mutation g)."""
    import math
    v, u = _stack(terms, "v"), _stack(terms, "u")
    keep = np.ones(len(index), bool)
    if drop is not None:
        keep[drop] = False
    shape = (n,) + v.shape[1:]
    val, unit, mag = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    np.add.at(unit, index, u)
    np.add.at(mag, index, np.abs(v))
    if exact:
        order = np.argsort(index[keep], kind="stable")
        vs, idx = v[keep][order].reshape(int(keep.sum()), -1), index[keep][order]
        ptr = np.searchsorted(idx, np.arange(n + 1))
        flat = val.reshape(n, -1)
        for g in range(n):
            if ptr[g + 1] > ptr[g]:
                flat[g] = [math.fsum(col) for col in vs[ptr[g]:ptr[g + 1]].T]
    else:
        np.add.at(val, index[keep], v[keep])
    return val, unit + EPS * mag


def ba_f64(cams, pp, pts, cam_idx, pt_idx, uv, loss_s=0.0, mut="", exact=False, drop=None):
    """The float64 restatement of the whole linearisation: (values, units), two dicts over
    BA_OUTPUTS (values also J [n,2,11], w, rho).  exact: sums by math.fsum.  drop: (mutation g) an
    observation left out of U."""
    import math
    T = ba_terms_f64(cams, pp, pts, cam_idx, pt_idx, uv, loss_s, mut)
    ci, pi = np.asarray(cam_idx, np.int64), np.asarray(pt_idx, np.int64)
    nc, npt = len(cams), len(pts)
    val, unit = {}, {}
    for k in ("res", "W"):
        val[k], unit[k] = _stack(T[k], "v"), _stack(T[k], "u")
    val["U"], unit["U"] = _segment(T["U"], ci, nc, exact, drop)
    val["gc"], unit["gc"] = _segment(T["gc"], ci, nc, exact)
    val["V"], unit["V"] = _segment(T["V"], pi, npt, exact)
    val["gp"], unit["gp"] = _segment(T["gp"], pi, npt, exact)
    h = T["hrho"]
    val["cost"] = math.fsum(h.v) if exact else float(np.sum(h.v))
    unit["cost"] = float(h.u.sum() + EPS * np.abs(h.v).sum())
    val.update(J=_stack(T["J"], "v"), w=T["w"].v, rho=T["rho"].v)
    unit.update(J=_stack(T["J"], "u"), rho=T["rho"].u, cost_sum=float(EPS * np.abs(h.v).sum()))
    return val, unit


def ba_units(cams, pp, pts, cam_idx, pt_idx, uv, loss_s=0.0):
    """The tolerance unit of every entry of res, W, U, V, gc, gp, cost (and J, rho; cost_sum: the
    summation part eps sum |rho / 2| alone)."""
    return ba_f64(cams, pp, pts, cam_idx, pt_idx, uv, loss_s)[1]


# ---- bundle-adjustment step solve -----------------------------------------------------------------
# Spec (include/sfmcore.h sfm_ba_solve, the header of csrc/ba_solve.hip): from the float64 blocks
# U, V, W, g_c, g_p (exact inputs here) and λ,
#   A_d = A + λ clamp(diag A, 1e-6, 1e32),  S = U_d - Σ_o W_o V_d⁻¹ W_oᵀ,  b = -g_c + Σ_o W_o V_d⁻¹ g_p,
#   S δc = b,  δp = V_d⁻¹ (-g_p - Σ_o W_oᵀ δc)  (δp = 0 for a point without observations),
#   model terms gᵀδ and δᵀ JᵀJ δ with the undamped blocks.
# Fixed parameters enter through the blocks (sfm_ba_fix_params / ba_lm.fix_params change them
# exactly), so the reference takes the blocks after that.

SOLVE_DIAG_MIN, SOLVE_DIAG_MAX = 1e-6, 1e32      # the float64 constants of the spec
SOLVE_CLASSES = (("r", slice(0, 3)), ("t", slice(3, 6)), ("f", slice(6, 7)), ("k1", slice(7, 8)))


def _mpl(a):
    """Nested lists of mpf from a float64 array."""
    a = np.asarray(a, np.float64)
    if a.ndim == 1:
        return [mp.mpf(float(x)) for x in a]
    return [_mpl(x) for x in a]


class SolveRef:
    """The 50-digit reference of one step solve (solve_blocks).  Attributes (float64 arrays unless
    said): Vinv [n_pt,3,3] (V_d⁻¹ rounded; zero for unobserved points), kappa [n_pt] = κ₂(V_d),
    ninv [n_pt] = ‖V_d⁻¹‖₂ (both 1 / 0 for unobserved points), b [n_cam,8]; 50-digit copies
    Vinv_hp, b_hp, Ud_hp.  Methods: S_mul, solve_residual, solve_backsub, solve_direct,
    model_terms and the units unit_backsub, unit_residual, unit_model."""

    @_hp
    def __init__(self, U, V, W, gc, gp, cam_idx, pt_idx, lam):
        f = lambda a, shape: np.ascontiguousarray(a, np.float64).reshape(shape)
        self.U, self.V, self.W = f(U, (-1, 8, 8)), f(V, (-1, 3, 3)), f(W, (-1, 8, 3))
        self.gc, self.gp = f(gc, (-1, 8)), f(gp, (-1, 3))
        self.ci = [int(c) for c in cam_idx]
        self.pi = [int(p) for p in pt_idx]
        self.nc, self.npt, self.no = len(self.U), len(self.V), len(self.ci)
        self.lam = float(lam)
        self.seen = np.bincount(np.asarray(self.pi, np.int64), minlength=self.npt) > 0
        lm = mp.mpf(self.lam)
        lo, hi = mp.mpf(SOLVE_DIAG_MIN), mp.mpf(SOLVE_DIAG_MAX)
        damp = lambda d: d + lm * min(max(d, lo), hi)
        self.U_hp, self.V_hp, self.W_hp = _mpl(self.U), _mpl(self.V), _mpl(self.W)
        self.gc_hp, self.gp_hp = _mpl(self.gc), _mpl(self.gp)
        self.Ud_hp = [[[damp(B[i][j]) if i == j else B[i][j] for j in range(8)] for i in range(8)]
                      for B in self.U_hp]
        zero = mp.mpf(0)
        self.Vinv_hp, self.kappa, self.ninv = [], np.ones(self.npt), np.zeros(self.npt)
        for p in range(self.npt):
            if not self.seen[p]:
                self.Vinv_hp.append([[zero] * 3 for _ in range(3)])
                continue
            B = self.V_hp[p]
            Vd = [[damp(B[i][j]) if i == j else B[i][j] for j in range(3)] for i in range(3)]
            self.Vinv_hp.append(_inv3(Vd))
            ev = sorted(abs(x) for x in mp.eigsy(mp.matrix(Vd), eigvals_only=True))
            self.kappa[p], self.ninv[p] = float(ev[2] / ev[0]), float(1 / ev[0])
        self.Vinv = np.array([[[float(x) for x in r] for r in B] for B in self.Vinv_hp]
                             ).reshape(self.npt, 3, 3)
        vg = [_mv(self.Vinv_hp[p], self.gp_hp[p]) for p in range(self.npt)]
        b = [[-x for x in g] for g in self.gc_hp]
        for o in range(self.no):
            Wo, v, bc = self.W_hp[o], vg[self.pi[o]], b[self.ci[o]]
            for i in range(8):
                bc[i] += Wo[i][0] * v[0] + Wo[i][1] * v[1] + Wo[i][2] * v[2]
        self.b_hp = b
        self.b = np.array([[float(x) for x in r] for r in b]).reshape(self.nc, 8)
        self.bnorm_hp = mp.sqrt(sum(x * x for r in b for x in r))
        self._direct = None

    # -- products ---------------------------------------------------------------------------
    def _wt(self, x):
        """Σ_o W_oᵀ x_c per point (x: [n_cam][8] of mpf)."""
        t = [[mp.mpf(0)] * 3 for _ in range(self.npt)]
        for o in range(self.no):
            Wo, xc, tp = self.W_hp[o], x[self.ci[o]], t[self.pi[o]]
            for j in range(3):
                s = tp[j]
                for i in range(8):
                    s += Wo[i][j] * xc[i]
                tp[j] = s
        return t

    @_hp
    def S_mul(self, x):
        """The implicit S·x = U_d x - Σ_o W_o V_d⁻¹ Σ_o' W_o'ᵀ x in 50 digits; x [n_cam, 8]
        float64 or nested mpf; returns nested mpf."""
        x = _mpl(x) if isinstance(x, np.ndarray) else x
        t = [_mv(self.Vinv_hp[p], tp) for p, tp in enumerate(self._wt(x))]
        y = [_mv(self.Ud_hp[c], x[c]) for c in range(self.nc)]
        for o in range(self.no):
            Wo, tp, yc = self.W_hp[o], t[self.pi[o]], y[self.ci[o]]
            for i in range(8):
                yc[i] -= Wo[i][0] * tp[0] + Wo[i][1] * tp[1] + Wo[i][2] * tp[2]
        return y

    @_hp
    def solve_residual(self, dc):
        """‖b - S·dc‖₂ / ‖b‖₂ for a float64 dc (0 when b = 0), as a float."""
        if self.bnorm_hp == 0:
            return 0.0
        y = self.S_mul(np.asarray(dc, np.float64).reshape(self.nc, 8))
        rr = sum((bi - yi) ** 2 for bc, yc in zip(self.b_hp, y) for bi, yi in zip(bc, yc))
        return float(mp.sqrt(rr) / self.bnorm_hp)

    @_hp
    def solve_backsub(self, dc, hp=False):
        """δp(dc) = V_d⁻¹ (-g_p - Σ_o W_oᵀ dc_c) per point for a float64 (or nested mpf) dc:
        float64 [n_pt, 3], or nested mpf with hp=True."""
        x = _mpl(np.asarray(dc, np.float64).reshape(self.nc, 8)) if not isinstance(dc, list) else dc
        t = self._wt(x)
        out = [_mv(self.Vinv_hp[p], [-g - s for g, s in zip(self.gp_hp[p], t[p])])
               for p in range(self.npt)]
        return out if hp else np.array([[float(v) for v in r] for r in out]).reshape(self.npt, 3)

    @_hp
    def backsub_error(self, dc, dp):
        """(‖dp - δp(dc)‖₂ per point with the difference taken in 50 digits, ‖δp(dc)‖₂ per point);
        a NaN or an infinity in dp gives inf."""
        ref = self.solve_backsub(dc, hp=True)
        dp = np.asarray(dp, np.float64).reshape(self.npt, 3)
        err, nrm = np.zeros(self.npt), np.zeros(self.npt)
        for p in range(self.npt):
            nrm[p] = float(mp.sqrt(sum(v * v for v in ref[p])))
            if not np.all(np.isfinite(dp[p])):
                err[p] = np.inf
                continue
            err[p] = float(mp.sqrt(sum((mp.mpf(float(a)) - v) ** 2 for a, v in zip(dp[p], ref[p]))))
        return err, nrm

    @_hp
    def solve_direct(self):
        """(δc* [n_cam, 8], δp* [n_pt, 3]) float64: dense S in 50 digits, mp.lu_solve, then the
        back-substitution of the 50-digit δc*.  Small problems only; cached."""
        if self._direct is None:
            assert self.nc <= 12, "solve_direct: small problems only"
            n = 8 * self.nc
            S = mp.zeros(n, n)
            for c in range(self.nc):
                for i in range(8):
                    for j in range(8):
                        S[8 * c + i, 8 * c + j] = self.Ud_hp[c][i][j]
            obs_of = [[] for _ in range(self.npt)]
            for o, p in enumerate(self.pi):
                obs_of[p].append(o)
            for p, obs in enumerate(obs_of):
                Vi = self.Vinv_hp[p]
                Y = {o: [[sum(self.W_hp[o][i][k] * Vi[k][j] for k in range(3)) for j in range(3)]
                         for i in range(8)] for o in obs}
                for a in obs:
                    ra = 8 * self.ci[a]
                    for b in obs:
                        rb, Wb = 8 * self.ci[b], self.W_hp[b]
                        for i in range(8):
                            Yi = Y[a][i]
                            for j in range(8):
                                S[ra + i, rb + j] -= Yi[0] * Wb[j][0] + Yi[1] * Wb[j][1] + Yi[2] * Wb[j][2]
            x = mp.lu_solve(S, mp.matrix([v for r in self.b_hp for v in r]))
            dc = [[x[8 * c + i] for i in range(8)] for c in range(self.nc)]
            dp = self.solve_backsub(dc, hp=True)
            self._direct = (np.array([[float(v) for v in r] for r in dc]).reshape(self.nc, 8),
                            np.array([[float(v) for v in r] for r in dp]).reshape(self.npt, 3))
        return self._direct

    def direct_error(self, dc, dp):
        """max |δ - δ*| / max |δ*| per parameter class (r, t, f, k1, X); a class whose δ* is all
        zero must be matched exactly (else inf); a NaN or an infinity gives inf."""
        sc, sp = self.solve_direct()
        dc, dp = np.asarray(dc, np.float64).reshape(sc.shape), np.asarray(dp, np.float64).reshape(sp.shape)
        out = {}
        for name, a, b in [(n, dc[:, s], sc[:, s]) for n, s in SOLVE_CLASSES] + [("X", dp, sp)]:
            if a.size == 0:
                continue
            d, m = np.abs(a - b).max(), np.abs(b).max()
            ok = np.all(np.isfinite(a))
            out[name] = float(d / m) if ok and m > 0 else (0.0 if ok and d == 0 else np.inf)
        return out

    @_hp
    def model_terms(self, dc, dp):
        """(gᵀδ, δᵀ JᵀJ δ) of a float64 δ with the undamped blocks, summed in 50 digits."""
        x = _mpl(np.asarray(dc, np.float64).reshape(self.nc, 8))
        y = _mpl(np.asarray(dp, np.float64).reshape(self.npt, 3)) if self.npt else []
        gd = sum(g * v for gr, xr in zip(self.gc_hp, x) for g, v in zip(gr, xr))
        gd += sum(g * v for gr, yr in zip(self.gp_hp, y) for g, v in zip(gr, yr))
        q = sum(xc[i] * sum(B[i][j] * xc[j] for j in range(8)) for B, xc in zip(self.U_hp, x)
                for i in range(8))
        q += sum(yp[i] * sum(B[i][j] * yp[j] for j in range(3)) for B, yp in zip(self.V_hp, y)
                 for i in range(3))
        for o in range(self.no):
            Wo, xc, yp = self.W_hp[o], x[self.ci[o]], y[self.pi[o]]
            q += 2 * sum(xc[i] * (Wo[i][0] * yp[0] + Wo[i][1] * yp[1] + Wo[i][2] * yp[2])
                         for i in range(8))
        return float(gd), float(q)

    @_hp
    def first_iterate(self):
        """The CG's first iterate x_1 = α M b, α = b·z / z·S z, z = M b, in 50 digits, with M as
        the spec states it: per camera the inverse of S_cc = U_d - Σ_o W_o V_d⁻¹ W_oᵀ over the
        camera's observations, or diag(1 / max(S_ii, 1e-6)) where a pivot of S_cc's Cholesky
        factorisation is not > 0.  Returns (x1 [n_cam, 8] float64, fallback [n_cam] bool,
        unit [n_cam]): unit_c = eps (κ₂(S_cc) + c_α) ‖x1_c‖₂, the forward error of a
        backward-stable solve with S_cc (κ = 1 for the diagonal form) plus the rounding of α,
        c_α = Σ|b_i z_i| / |b·z| + Σ|z_i (S z)_i| / |z·S z|."""
        S = [[row[:] for row in B] for B in self.Ud_hp]
        for o in range(self.no):
            Wo, Vi, Sc = self.W_hp[o], self.Vinv_hp[self.pi[o]], S[self.ci[o]]
            Y = [_mv([[Vi[k][j] for k in range(3)] for j in range(3)], Wo[i]) for i in range(8)]
            for i in range(8):
                for j in range(8):
                    Sc[i][j] -= Y[i][0] * Wo[j][0] + Y[i][1] * Wo[j][1] + Y[i][2] * Wo[j][2]
        lo = mp.mpf(SOLVE_DIAG_MIN)
        z, bad, kap = [], np.zeros(self.nc, bool), np.ones(self.nc)
        for c in range(self.nc):
            A = mp.matrix(S[c])
            L = mp.zeros(8, 8)
            for j in range(8):
                sv = A[j, j] - sum(L[j, k] ** 2 for k in range(j))
                if not sv > 0:
                    bad[c] = True
                    break
                L[j, j] = mp.sqrt(sv)
                for i in range(j + 1, 8):
                    L[i, j] = (A[i, j] - sum(L[i, k] * L[j, k] for k in range(j))) / L[j, j]
            if bad[c]:
                z.append([self.b_hp[c][i] / max(S[c][i][i], lo) for i in range(8)])
            else:
                z.append(list(mp.lu_solve(A, mp.matrix(self.b_hp[c]))))
                ev = sorted(abs(x) for x in mp.eigsy(A, eigvals_only=True))
                kap[c] = float(ev[-1] / ev[0])
        q = self.S_mul(z)
        bz = [bi * zi for bc, zc in zip(self.b_hp, z) for bi, zi in zip(bc, zc)]
        zq = [zi * qi for zc, qc in zip(z, q) for zi, qi in zip(zc, qc)]
        alpha = sum(bz) / sum(zq)
        c_alpha = float(sum(abs(t) for t in bz) / abs(sum(bz)) + sum(abs(t) for t in zq) / abs(sum(zq)))
        x1 = np.array([[float(alpha * v) for v in zc] for zc in z]).reshape(self.nc, 8)
        return x1, bad, EPS * (kap + c_alpha) * np.linalg.norm(x1, axis=1)

    # -- units (float64: a unit needs no more) -------------------------------------------------
    def unit_backsub(self, dc, ref_norm):
        """u_p = eps (κ₂(V_d) ‖δp_ref‖₂ + ‖V_d⁻¹‖₂ (‖g_p‖₁ + Σ_o ‖|W_o|ᵀ|dc_c|‖₁)) per point: the
        forward error of a backward-stable 3x3 solve plus the rounding of its right-hand side."""
        a = np.abs(np.asarray(dc, np.float64).reshape(self.nc, 8))
        rhs = np.abs(self.gp).sum(1)
        if self.no:
            np.add.at(rhs, np.asarray(self.pi), np.einsum("oij,oi->oj", np.abs(self.W),
                                                          a[np.asarray(self.ci)]).sum(1))
        return EPS * (self.kappa * np.asarray(ref_norm) + self.ninv * rhs)

    def unit_residual(self, dc):
        """u_r = eps ‖ |U_d||dc| + Σ |W||V_d⁻¹||W|ᵀ|dc| + |b| ‖₂ / ‖b‖₂: one rounding of one
        evaluation of b - S·dc (0 when b = 0)."""
        bn = float(self.bnorm_hp)
        if bn == 0.0:
            return 0.0
        a = np.abs(np.asarray(dc, np.float64).reshape(self.nc, 8))
        Ud = np.abs(np.array([[[float(v) for v in r] for r in B] for B in self.Ud_hp]))
        v = np.einsum("cij,cj->ci", Ud.reshape(self.nc, 8, 8), a) + np.abs(self.b)
        if self.no:
            ci, pi, Wa = np.asarray(self.ci), np.asarray(self.pi), np.abs(self.W)
            t = np.zeros((self.npt, 3))
            np.add.at(t, pi, np.einsum("oij,oi->oj", Wa, a[ci]))
            t = np.einsum("pij,pj->pi", np.abs(self.Vinv), t)
            np.add.at(v, ci, np.einsum("oij,oj->oi", Wa, t[pi]))
        return EPS * float(np.sqrt((v * v).sum())) / bn

    def unit_model(self, dc, dp):
        """(eps Σ|term| of gᵀδ, eps Σ|term| of δᵀ JᵀJ δ)."""
        a = np.abs(np.asarray(dc, np.float64).reshape(self.nc, 8))
        d = np.abs(np.asarray(dp, np.float64).reshape(self.npt, 3))
        gd = (np.abs(self.gc) * a).sum() + (np.abs(self.gp) * d).sum()
        q = np.einsum("ci,cij,cj->", a, np.abs(self.U), a) + np.einsum("pi,pij,pj->", d, np.abs(self.V), d)
        if self.no:
            q += 2.0 * np.einsum("oi,oij,oj->", a[np.asarray(self.ci)], np.abs(self.W),
                                 d[np.asarray(self.pi)])
        return EPS * float(gd), EPS * float(q)


def _mv(A, x):
    return [sum(a * v for a, v in zip(row, x)) for row in A]


def _inv3(A):
    """Inverse of a 3x3 nested-mpf matrix (adjugate / determinant: exact enough at 50 digits)."""
    (a, b, c), (d, e, f), (g, h, i) = A
    C = [[e * i - f * h, c * h - b * i, b * f - c * e],
         [f * g - d * i, a * i - c * g, c * d - a * f],
         [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = a * C[0][0] + b * C[1][0] + c * C[2][0]
    return [[x / det for x in row] for row in C]


def solve_blocks(U, V, W, gc, gp, cam_idx, pt_idx, lam):
    """The 50-digit reference of sfm_ba_solve on the float64 blocks (after any fix_params)."""
    return SolveRef(U, V, W, gc, gp, cam_idx, pt_idx, lam)


# Float64 restatement of the whole solve (written from the spec, numpy), with the mutations of the
# mutation check in tests/test_ba_solve_hp_cpu.py; mut is never set otherwise.
SOLVE_MUTATIONS = dict(
    a="damping without the clamp", b="W_o read as its transpose's layout in the CG point sum",
    c="one observation of the 257-track dropped from the back-substitution's sum",
    d="a 65-observation point's dp left at its set-up value -V_d^-1 g_p",
    e="S p with the undamped U", f="+g_p for -g_p in the back-substitution",
    g="the last camera's z = M r skipped", h="info[1] forced to 0 on a breakdown")


def solve_f64(U, V, W, gc, gp, cam_idx, pt_idx, lam, max_iter=100, tol=1e-10, mut=""):
    """(dc, dp, info [5]) as sfm_ba_solve returns them: fallback, breakdown and info as the spec
    states them.  mut: a key of SOLVE_MUTATIONS."""
    U, V, W = (np.asarray(a, np.float64) for a in (U, V, W))
    gc, gp = np.asarray(gc, np.float64), np.asarray(gp, np.float64)
    ci, pi = np.asarray(cam_idx, np.int64), np.asarray(pt_idx, np.int64)
    nc, npt = len(U), len(V)
    cnt = np.bincount(pi, minlength=npt)

    def damp(A):
        d = np.diagonal(A, axis1=-2, axis2=-1)
        d = d if mut == "a" else np.clip(d, SOLVE_DIAG_MIN, SOLVE_DIAG_MAX)
        out = A.copy()
        k = np.arange(A.shape[-1])
        out[..., k, k] += lam * d
        return out

    Vinv = np.zeros_like(V)
    if (cnt > 0).any():
        Vinv[cnt > 0] = np.linalg.inv(damp(V)[cnt > 0])
    vg = np.einsum("pij,pj->pi", Vinv, gp)
    Ud = damp(U)
    Wt = W.reshape(-1, 3, 8).transpose(0, 2, 1) if mut == "b" else W

    def wt(x, Wm=W, skip=None):
        t = np.zeros((npt, 3))
        term = np.einsum("oij,oi->oj", Wm, x[ci])
        if skip is not None:
            term[skip] = 0.0
        np.add.at(t, pi, term)
        return t

    def smul(x):
        t = np.einsum("pij,pj->pi", Vinv, wt(x, Wt))
        y = np.einsum("cij,cj->ci", U if mut == "e" else Ud, x)
        np.subtract.at(y, ci, np.einsum("oij,oj->oi", W, t[pi]))
        return y

    Scc = Ud.copy()
    np.subtract.at(Scc, ci, np.einsum("oik,ojk->oij", np.einsum("oij,ojk->oik", W, Vinv[pi]), W))
    b = -gc.copy()
    np.add.at(b, ci, np.einsum("oij,oj->oi", W, vg[pi]))
    M, flag = np.zeros_like(Scc), 0
    for c in range(nc):
        try:
            np.linalg.cholesky(Scc[c])
            M[c] = np.linalg.inv(Scc[c])
        except np.linalg.LinAlgError:
            M[c] = np.diag(1.0 / np.maximum(np.diag(Scc[c]), SOLVE_DIAG_MIN))
            flag |= 1

    def precond(r, z_old):
        z = np.einsum("cij,cj->ci", M, r)
        if mut == "g" and z_old is not None:
            z[-1] = z_old[-1]
        return z

    x, r = np.zeros_like(b), b.copy()
    bb = float((b * b).sum())
    z = precond(r, None)
    p, rz, rr, it = z.copy(), float((r * z).sum()), bb, 0
    broke = False
    while it < max_iter and bb > 0.0 and rr > tol * tol * bb:
        q = smul(p)
        pq = float((p * q).sum())
        it += 1
        if not pq > 0.0:
            flag |= 2
            broke = True
            break
        al = float(np.float64(rz) / np.float64(pq))
        x += al * p
        r -= al * q
        rr = float((r * r).sum())
        z = precond(r, z)
        rz_new = float((r * z).sum())
        with np.errstate(all="ignore"):           # a mutation may end in 0 / 0: as the kernel, NaN
            p = z + (np.float64(rz_new) / np.float64(rz)) * p
        rz = rz_new
    keep = None
    if mut == "c":
        long = np.nonzero(cnt == 257)[0]
        keep = int(np.nonzero(pi == long[0])[0][100]) if len(long) else None
    sign = 1.0 if mut == "f" else -1.0
    dp = sign * vg - np.einsum("pij,pj->pi", Vinv, wt(x, W, keep))
    if mut == "d":
        sel = np.nonzero(cnt == 65)[0]
        dp[sel[:1]] = -vg[sel[:1]]
    gd = float((gc * x).sum() + (gp * dp).sum())
    qq = float(np.einsum("ci,cij,cj->", x, U, x) + np.einsum("pi,pij,pj->", dp, V, dp)
               + 2.0 * np.einsum("oi,oij,oj->", x[ci], W, dp[pi]))
    rel = np.sqrt(rr / bb) if bb > 0.0 else 0.0
    if mut == "h" and broke:
        rel = 0.0
    return x, dp, np.array([it, rel, gd, qq, flag], np.float64)


# ---- two-view relative pose -----------------------------------------------------------------------
# Spec (header of csrc/two_view_pose.hip): undistorted coordinates by 10 fixed-point
# steps; N = A^T A over the inliers, E its null vector; the four (R, t) from E's SVD; the depth
# numerators l1 = (a.b)(b.t) - (a.t)(b.b), l2 = (a.a)(b.t) - (a.b)(a.t) with a = R (x1, 1),
# b = (x2, 1); the key s = |a x b|^2 / ((a.a)(b.b)) for a.b >= 0, else 2 - s, rounded to float32.
# Every function takes float64 inputs, so a comparison charges the code only with its own error.

POSE_TINY = 1e-8
POSE_SWEEPS = 30


@_hp
def undistort_exact(xd, k1):
    """The true inverse of x (1 + k1 |x|^2) = xd: (x [2] of mpf, rho), rho = |2 k1 r^2 / (1 + k1 r^2)|
    the contraction factor of the fixed-point map x <- xd / (1 + k1 |x|^2) at the solution; (None,
    None) where no inverse exists (k1 < 0 and |xd| beyond the fold 2 / (3 sqrt(-3 k1))).  Newton on
    the radial cubic r + k1 r^3 = |xd| from the side on which it converges monotonically; of the
    roots for k1 < 0 the one on the branch through the origin."""
    xd = _vec(xd)
    k1 = mp.mpf(float(k1))
    rd = mp.sqrt(xd[0] * xd[0] + xd[1] * xd[1])
    if rd == 0:
        return [mp.mpf(0), mp.mpf(0)], mp.mpf(0)
    if k1 < 0:
        rs = 1 / mp.sqrt(-3 * k1)
        if rd > 2 * rs / 3:
            return None, None
        r = mp.mpf(0)           # concave: from the left
    else:
        r = rd                  # convex: from the right
    for _ in range(200):
        step = (r + k1 * r ** 3 - rd) / (1 + 3 * k1 * r * r)
        r -= step
        if abs(step) <= mp.mpf(10) ** (-DPS + 5) * rd:
            break
    rho = abs(2 * k1 * r * r / (1 + k1 * r * r))
    return [xd[0] * r / rd, xd[1] * r / rd], rho


@_hp
def undistort_steps(xd, k1, n=UNDISTORT_ITERS):
    """The spec's n fixed-point steps in 50 digits: (x [2] of mpf, unit), the unit being the
    first-order float64 error of the same steps: u <- |dT/dr| u + eps |x| (2 + 3 |k1| r^2 / |s|)."""
    xd = _vec(xd)
    k1 = mp.mpf(float(k1))
    x0, x1 = xd
    u = mp.mpf(0)
    for _ in range(n):
        r2 = x0 * x0 + x1 * x1
        s = 1 + k1 * r2
        y0, y1 = xd[0] / s, xd[1] / s
        ny = mp.sqrt(y0 * y0 + y1 * y1)
        u = abs(2 * k1 * mp.sqrt(r2) * ny / s) * u + EPS * ny * (2 + 3 * abs(k1) * r2 / abs(s))
        x0, x1 = y0, y1
    return [x0, x1], float(u)


def _pose_rows(x1, x2, mask):
    x1 = np.asarray(x1, np.float64).reshape(-1, 2)
    x2 = np.asarray(x2, np.float64).reshape(-1, 2)
    on = np.ones(len(x1), bool) if mask is None else np.asarray(mask).astype(bool)[:len(x1)]
    rows = []
    for a, b in zip(_mpl(x1[on]), _mpl(x2[on])):
        rows.append([b[0] * a[0], b[0] * a[1], b[0], b[1] * a[0], b[1] * a[1], b[1], a[0], a[1],
                     mp.mpf(1)])
    return rows


@_hp
def pose_normal(x1, x2, mask=None):
    """The fit in 50 digits.  dict: N [9,9] (the exact sum, rounded; N_mp unrounded, T_mp the sums
    of the absolute terms), unit [9,9] = eps sum |terms|,
    lam [9] ascending eigenvalues of the exact N, gap = lam2 - lam1, e [9] its null vector (mpf);
    sv [9] ascending singular values of A itself, sgap = sv2 - sv1, a_null [9] A's null vector
    (mp.svd_r; fewer than nine rows are padded with zero rows)."""
    rows = _pose_rows(x1, x2, mask)
    N, T = mp.zeros(9, 9), mp.zeros(9, 9)
    for r in rows:
        for i in range(9):
            for j in range(i, 9):
                N[i, j] += r[i] * r[j]
                T[i, j] += abs(r[i] * r[j])
    for i in range(9):
        for j in range(i):
            N[i, j], T[i, j] = N[j, i], T[j, i]
    ev, Q = mp.eigsy(N)
    order = sorted(range(9), key=lambda k: ev[k])
    lam = [ev[k] for k in order]
    A = mp.matrix(rows + [[0] * 9] * max(0, 9 - len(rows)))
    _, S, V = mp.svd_r(A, full_matrices=False, compute_uv=True)
    so = sorted(range(9), key=lambda k: S[k])
    sv = [S[k] for k in so]
    f = lambda M: np.array([[float(M[i, j]) for j in range(9)] for i in range(9)])
    return dict(N=f(N), unit=EPS * f(T), N_mp=N, T_mp=T, lam=np.array([float(x) for x in lam]),
                gap=float(lam[1] - lam[0]), e=[Q[i, order[0]] for i in range(9)],
                sv=np.array([float(x) for x in sv]), sgap=float(sv[1] - sv[0]),
                a_null=[V[so[0], j] for j in range(9)])


@_hp
def normal_ratio(N, ref):
    """Worst |N - exact N| / (eps sum |terms|) over the entries of a float64 N [9,9]; ref from
    pose_normal.  An entry without terms must be exactly zero."""
    N = np.asarray(N, np.float64).reshape(9, 9)
    worst = mp.mpf(0)
    for i in range(9):
        for j in range(9):
            if not np.isfinite(N[i, j]):
                return np.inf
            d, u = abs(mp.mpf(float(N[i, j])) - ref["N_mp"][i, j]), EPS * ref["T_mp"][i, j]
            if u == 0:
                if d != 0:
                    return np.inf
                continue
            worst = max(worst, d / u)
    return float(worst)


@_hp
def norm_minus_1(v):
    v = _vec(np.asarray(v, np.float64).ravel())
    return float(mp.sqrt(sum(x * x for x in v)) - 1)


@_hp
def orth_defect(R, t):
    """max(|R^T R - I|, |det R - 1|, ||t| - 1|) of a float64 (R [9], t [3]), formed in 50 digits."""
    R = _mpl(np.asarray(R, np.float64).reshape(3, 3))
    d = max(abs(sum(R[k][i] * R[k][j] for k in range(3)) - (1 if i == j else 0))
            for i in range(3) for j in range(3))
    c = _cross(R[1], R[2])
    det = R[0][0] * c[0] + R[0][1] * c[1] + R[0][2] * c[2]
    return float(max(d, abs(det - 1), abs(norm_minus_1(t))))


@_hp
def key_bracket(key_mp, half):
    """(lo, hi) f32 arrays: the exact keys minus / plus `half`, each rounded once to float32."""
    lo = np.array([_to_f32(k - mp.mpf(float(h))) for k, h in zip(key_mp, half)], np.float32)
    hi = np.array([_to_f32(k + mp.mpf(float(h))) for k, h in zip(key_mp, half)], np.float32)
    return lo, hi


@_hp
def undistort_compare(xd, k1, x, x_numpy, f=1000.0):
    """One keypoint: the spec's output x (float64) and a plain numpy run of the same steps against
    undistort_steps and undistort_exact.  dict exists, rho, px (|x - exact| f), steps (|x - steps| /
    its unit), exact and numpy (|. - exact| / ((eps + rho^10) |x|))."""
    xs, us = undistort_steps(xd, k1)
    xe, rho = undistort_exact(xd, k1)
    dist = lambda a, b: mp.sqrt((mp.mpf(float(a[0])) - b[0]) ** 2 + (mp.mpf(float(a[1])) - b[1]) ** 2)
    ds = dist(x, xs)
    out = dict(exists=xe is not None, rho=float(rho) if xe is not None else np.nan,
               steps=float(ds / us) if us > 0 else (0.0 if ds == 0 else np.inf),
               px=np.nan, exact=np.nan, numpy=np.nan)
    if xe is not None:
        nx = mp.sqrt(xe[0] ** 2 + xe[1] ** 2)
        unit = (EPS + rho ** UNDISTORT_ITERS) * nx
        de, dn = dist(x, xe), dist(x_numpy, xe)
        out["px"] = float(de * f)
        out["exact"] = float(de / unit) if unit > 0 else (0.0 if de == 0 else np.inf)
        out["numpy"] = float(dn / unit) if unit > 0 else (0.0 if dn == 0 else np.inf)
    return out


def vec_dist(v, ref):
    """max |v -+ ref| up to sign; v float64, ref a list of mpf."""
    with mp.workdps(DPS):
        v = _vec(np.asarray(v, np.float64).ravel())
        return float(min(max(abs(a - b) for a, b in zip(v, ref)),
                         max(abs(a + b) for a, b in zip(v, ref))))


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


@_hp
def pose_decompose(E):
    """50-digit SVD of a float64 E [9] and the spec's four candidates.  dict: sigma [3] descending,
    cands = [(R 3x3 of mpf, t [3] of mpf)] x 4 (as a set: the order depends on the signs of the
    singular vectors), status2 (a column norm of U at or below POSE_TINY), unit = eps sigma1 /
    (sigma2 - sigma3), the conditioning of R and t."""
    M = mp.matrix(3, 3)
    for i, x in enumerate(np.asarray(E, np.float64).ravel()):
        M[i // 3, i % 3] = mp.mpf(float(x))
    U, S, V = mp.svd_r(M, full_matrices=True, compute_uv=True)
    o = sorted(range(3), key=lambda k: -S[k])
    sg = [S[k] for k in o]
    v1, v2 = [V[o[0], j] for j in range(3)], [V[o[1], j] for j in range(3)]
    u1, u2 = [U[i, o[0]] for i in range(3)], [U[i, o[1]] for i in range(3)]
    v3, u3 = _cross(v1, v2), _cross(u1, u2)
    Ra = [[u2[i] * v1[j] - u1[i] * v2[j] + u3[i] * v3[j] for j in range(3)] for i in range(3)]
    Rb = [[u1[i] * v2[j] - u2[i] * v1[j] + u3[i] * v3[j] for j in range(3)] for i in range(3)]
    neg = [-x for x in u3]
    gap = sg[1] - sg[2]
    return dict(sigma=np.array([float(x) for x in sg]),
                cands=[(Ra, u3), (Ra, neg), (Rb, u3), (Rb, neg)],
                status2=bool(sg[0] <= POSE_TINY or sg[1] <= POSE_TINY),
                unit=float(EPS * sg[0] / gap) if gap > 0 else np.inf)


def pose_dist(R, t, cands):
    """Distance of a float64 (R, t) from the nearest 50-digit candidate: max over the 12 entries."""
    with mp.workdps(DPS):
        R, t = _vec(np.asarray(R, np.float64).ravel()), _vec(t)
        best = None
        for Rc, tc in cands:
            d = max(max(abs(R[3 * i + j] - Rc[i][j]) for i in range(3) for j in range(3)),
                    max(abs(t[i] - tc[i]) for i in range(3)))
            best = d if best is None or d < best else best
        return float(best)


def pose_vote(R, t, x1, x2, mask=None):
    """Per masked-in match under a float64 (R, t), in 50 digits: dict of float64 arrays l1, l2, ab,
    key (exact, rounded to float64; key_mp unrounded), key32 (rounded once to float32), and the first-order
    float64 error units u_l1, u_l2, u_key (eps times the sum of the absolute terms, hp_ref.VU),
    front (both numerators > 0)."""
    x1 = np.asarray(x1, np.float64).reshape(-1, 2)
    x2 = np.asarray(x2, np.float64).reshape(-1, 2)
    on = np.ones(len(x1), bool) if mask is None else np.asarray(mask).astype(bool)[:len(x1)]
    x1, x2 = x1[on], x2[on]
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64)
    n = len(x1)
    # units: the float64 evaluation with exact inputs
    c = lambda v: VU(np.full(n, float(v)))
    p, q = [VU(x1[:, 0]), VU(x1[:, 1])], [VU(x2[:, 0]), VU(x2[:, 1]), c(1.0)]
    a = [vsum([c(R[i, 0]) * p[0], c(R[i, 1]) * p[1], c(R[i, 2])]) for i in range(3)]
    tv = [c(t[i]) for i in range(3)]
    dot = lambda u, v: vsum([u[0] * v[0], u[1] * v[1], u[2] * v[2]])
    aa, bb, ab, at, bt = dot(a, a), dot(q, q), dot(a, q), dot(a, tv), dot(q, tv)
    l1 = vsum([ab * bt, -(at * bb)])
    l2 = vsum([aa * bt, -(ab * at)])
    cr = [vsum([a[1] * q[2], -(a[2] * q[1])]), vsum([a[2] * q[0], -(a[0] * q[2])]),
          vsum([a[0] * q[1], -(a[1] * q[0])])]
    s = dot(cr, cr) / (aa * bb)
    u_key = np.where(ab.v >= 0.0, s.u, s.u + EPS * np.abs(2.0 - s.v))
    out = dict(u_l1=l1.u, u_l2=l2.u, u_key=u_key)
    ex = {k: np.zeros(n) for k in ("l1", "l2", "ab", "key")}
    k32, key_mp = np.zeros(n, np.float32), []
    with mp.workdps(DPS):
        Rm, tm = _mpl(R), _mpl(t)
        for m, (xa, xb) in enumerate(zip(_mpl(x1), _mpl(x2))):
            am = [Rm[i][0] * xa[0] + Rm[i][1] * xa[1] + Rm[i][2] for i in range(3)]
            bm = [xb[0], xb[1], mp.mpf(1)]
            d = lambda u, v: u[0] * v[0] + u[1] * v[1] + u[2] * v[2]
            maa, mbb, mab, mat, mbt = d(am, am), d(bm, bm), d(am, bm), d(am, tm), d(bm, tm)
            cm = _cross(am, bm)
            ms = d(cm, cm) / (maa * mbb)
            key = ms if mab >= 0 else 2 - ms
            ex["l1"][m], ex["l2"][m] = float(mab * mbt - mat * mbb), float(maa * mbt - mab * mat)
            ex["ab"][m], ex["key"][m] = float(mab), float(key)
            k32[m] = _to_f32(key)
            key_mp.append(key)
    out.update(ex)
    out["key_mp"] = key_mp
    out["key32"] = k32
    out["front"] = (ex["l1"] > 0) & (ex["l2"] > 0)
    return out


def _to_f32(x):
    """An mpf rounded ONCE to float32 (not through float64: no double rounding)."""
    if x == 0:
        return np.float32(0.0)
    with mp.workprec(24):
        y = +x
    return np.float32(float(y))


# Float64 restatement of the whole spec (numpy, written from DESIGN §4.2b), with the mutations of the
# mutation check in tests/test_two_view_pose_hp_cpu.py; mut is never set otherwise.
POSE_MUTATIONS = dict(
    a="Jacobi capped at 2 sweeps", b="the second-smallest eigenvector taken",
    c="the sign rule of tt dropped for theta < 0", d="the Gram-Schmidt step of u2 skipped",
    e="at and bt swapped in l2", f="the 2 - s branch dropped",
    g="upper median for lower median", h="> turned into >= at wide_key")


def _jacobi_f64(A, mut=""):
    """Cyclic Jacobi in the spec's round-robin order: (diagonal, V)."""
    A = np.array(A, np.float64)
    n = len(A)
    V = np.eye(n)
    h = (n - 1) // 2
    for _ in range(2 if mut == "a" else POSE_SWEEPS):
        off = float((np.triu(A, 1) ** 2).sum())
        tr = float(np.trace(A))
        if off <= 1e-60 * tr * tr:
            break
        for r in range(n):
            rot = []
            for i in range(h):
                a, b = (r + i + 1) % n, (r + n - i - 1) % n
                p, q = min(a, b), max(a, b)
                c, s = 1.0, 0.0
                if abs(A[p, q]) > 1e-300:
                    th = (A[q, q] - A[p, p]) / (2.0 * A[p, q])
                    sg = 1.0 if (th >= 0.0 or mut == "c") else -1.0
                    tt = sg / (abs(th) + np.sqrt(th * th + 1.0))
                    c = 1.0 / np.sqrt(tt * tt + 1.0)
                    s = tt * c
                rot.append((p, q, c, s))
            for p, q, c, s in rot:
                for M in (A, V):
                    mp_, mq_ = M[:, p].copy(), M[:, q].copy()
                    M[:, p], M[:, q] = c * mp_ - s * mq_, s * mp_ + c * mq_
            for p, q, c, s in rot:
                rp, rq = A[p].copy(), A[q].copy()
                A[p], A[q] = c * rp - s * rq, s * rp + c * rq
    return np.diag(A).copy(), V


def score_f64(R, t, x1, x2, mut=""):
    """(l1, l2, key f32) of every match under (R, t), numpy float64 in the spec's order of
    operations."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    a = [(R[i, 0] * x1[:, 0] + R[i, 1] * x1[:, 1]) + R[i, 2] for i in range(3)]
    b = [x2[:, 0], x2[:, 1], np.ones(len(x2))]
    dot = lambda u, v: (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]
    aa, bb, ab = dot(a, a), dot(b, b), dot(a, b)
    at, bt = dot(a, [t[0], t[1], t[2]]), dot(b, [t[0], t[1], t[2]])
    l1 = ab * bt - at * bb
    l2 = (aa * at - ab * bt) if mut == "e" else (aa * bt - ab * at)
    c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    s = dot(c, c) / (aa * bb)
    key = s if mut == "f" else np.where(ab >= 0.0, s, 2.0 - s)
    return l1, l2, key.astype(np.float32)


def decompose_f64(E, mut=""):
    """(Ra, Rb, u3, ok) of a float64 E [9] as the spec decomposes it."""
    E = np.asarray(E, np.float64).reshape(3, 3)
    G = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            G[i, j] = (E[0, i] * E[0, j] + E[1, i] * E[1, j]) + E[2, i] * E[2, j]
    w, V = _jacobi_f64(G, mut)
    i1 = 0
    for k in (1, 2):
        if w[k] > w[i1]:
            i1 = k
    i2 = 1 if i1 == 0 else 0
    for k in range(i2 + 1, 3):
        if k != i1 and w[k] > w[i2]:
            i2 = k
    v1, v2 = V[:, i1], V[:, i2]
    v3 = np.cross(v1, v2)
    u1, u2 = E @ v1, E @ v2
    n1 = np.sqrt(u1 @ u1)
    if not n1 > POSE_TINY:
        return None, None, None, False
    u1 = u1 / n1
    if mut != "d":
        u2 = u2 - (u2 @ u1) * u1
    n2 = np.sqrt(u2 @ u2)
    if not n2 > POSE_TINY:
        return None, None, None, False
    u2 = u2 / n2
    u3 = np.cross(u1, u2)
    Ra = np.outer(u2, v1) - np.outer(u1, v2) + np.outer(u3, v3)
    Rb = np.outer(u1, v2) - np.outer(u2, v1) + np.outer(u3, v3)
    return Ra, Rb, u3, True


def pose_f64(x1, x2, mask=None, mut="", min_inliers=8, wide_key=0.0):
    """dict(E [9], R [9], t [3], stat [8], median_key f32, N [9,9], cand (Ra, Rb, u3)) as
    tests/pose_ref.c returns them.  mut: a key of POSE_MUTATIONS."""
    x1 = np.asarray(x1, np.float64).reshape(-1, 2)
    x2 = np.asarray(x2, np.float64).reshape(-1, 2)
    on = np.ones(len(x1), bool) if mask is None else np.asarray(mask).astype(bool)[:len(x1)]
    x1, x2 = x1[on], x2[on]
    n = len(x1)
    out = dict(E=np.zeros(9), R=np.zeros(9), t=np.zeros(3), stat=np.zeros(8, np.int32),
               median_key=np.float32(0.0), N=np.zeros((9, 9)), cand=None)
    if n < max(min_inliers, 8):
        out["stat"][0] = 1
        return out
    A = np.stack([x2[:, 0] * x1[:, 0], x2[:, 0] * x1[:, 1], x2[:, 0], x2[:, 1] * x1[:, 0],
                  x2[:, 1] * x1[:, 1], x2[:, 1], x1[:, 0], x1[:, 1], np.ones(n)], 1)
    N = np.zeros((9, 9))
    for i in range(9):
        for j in range(i, 9):
            N[i, j] = N[j, i] = float(np.sum(A[:, i] * A[:, j]))
    out["N"] = N
    w, V = _jacobi_f64(N, mut)
    order = np.argsort(w, kind="stable")
    e = V[:, order[1] if mut == "b" else order[0]].copy()
    Ra, Rb, u3, ok = decompose_f64(e, mut)
    if not ok:
        out["stat"][0] = 2
        return out
    out["cand"] = (Ra, Rb, u3)
    nf, keys = [], []
    for c in range(4):
        Rc, tc = (Rb if c >> 1 else Ra), (-u3 if c & 1 else u3)
        l1, l2, key = score_f64(Rc, tc, x1, x2, mut)
        front = (l1 > 0.0) & (l2 > 0.0)
        nf.append(int(front.sum()))
        keys.append(np.sort(key[front]))
    best = int(np.argmax(nf))
    k = keys[best]
    wk = np.float32(wide_key)
    out["E"], out["R"] = e, (Rb if best >> 1 else Ra).ravel().copy()
    out["t"] = (-u3 if best & 1 else u3).copy()
    n_wide = int((k >= wk).sum() if mut == "h" else (k > wk).sum())
    out["stat"][:] = [0, best, *nf, n_wide, n]
    if len(k):
        out["median_key"] = k[len(k) // 2 if mut == "g" else (len(k) - 1) // 2]
    return out
