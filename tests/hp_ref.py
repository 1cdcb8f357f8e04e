"""50-digit references for the steps after the match graph (test infrastructure, mpmath).

Written from the specs in the kernel headers (csrc/camera_model.h, csrc/triangulate.hip), not from
the kernels: every quantity is formed in 50-digit arithmetic from the float64 inputs, so the only
error a comparison charges to the code under test is its own.

  rotmat(r)                                   Rodrigues; the spec's first-order form for |r|^2 <= 1e-20
  rot_err(r_out, R_ref)                       max |rotmat(r_out) - R_ref|
  exp_so3(axis, theta)                        exp(theta [a]x) for a unit axis given in 50 digits
  triangulate(cams, pp, pt_ptr, cam_idx, uv)  multi-view DLT, statistics, status, eigenvalues
  stats_f64(...)                              the three statistics at a given X, float64 (for
                                              propagating a point tolerance to the statistics)
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
