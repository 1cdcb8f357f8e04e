"""Seeded two-view cases for the homography / two-view-geometry tests (numpy only).

Two cameras at -0.1 and +0.1 rad on the radius-8 circle around the y axis, at heights -0.02*8 and
+0.02*8, looking at the origin; f = 1000, principal point (960, 540).  n points uniform in
[-2, 2]^3, N(0, noise) pixel noise in both images, and the first `outlier_frac` of the image-2
points replaced by uniform outliers in 1920x1080.  Kinds:
  "general"  the 3-D box
  "plane"    z = 0.3 x - 0.2 y
  "rot"      camera 2 at camera 1's centre with R2 = R_y(0.08) R1 (pure rotation)
"""
from __future__ import annotations

import numpy as np

import synth

KINDS = ("general", "plane", "rot")
F_PX, PP = 1000.0, (960.0, 540.0)
W, H = 1920, 1080
K = np.array([[F_PX, 0, PP[0]], [0, F_PX, PP[1]], [0, 0, 1.0]])
PLANE_A = np.array([[1.0, 0, 0], [0, 1.0, 0], [0.3, -0.2, 0]])  # (x, y, 1) -> point on the plane


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]])


def cameras(kind):
    """(R1, t1, R2, t2), world -> camera."""
    C1 = 8.0 * np.array([np.sin(-0.1), -0.02, np.cos(-0.1)])
    C2 = 8.0 * np.array([np.sin(0.1), 0.02, np.cos(0.1)])
    R1 = synth._look_at(C1)
    if kind == "rot":
        R2, C2 = _rot_y(0.08) @ R1, C1
    else:
        R2 = synth._look_at(C2)
    return R1, -R1 @ C1, R2, -R2 @ C2


def true_homography(kind):
    """Pixel homography image 1 -> image 2 of the "plane" and "rot" kinds (unnormalised)."""
    R1, t1, R2, t2 = cameras(kind)
    if kind == "rot":
        return K @ R2 @ R1.T @ np.linalg.inv(K)
    assert kind == "plane"
    e3 = np.array([[0, 0, 1.0]])
    P1 = K @ (R1 @ PLANE_A + t1[:, None] @ e3)
    P2 = K @ (R2 @ PLANE_A + t2[:, None] @ e3)
    return P2 @ np.linalg.inv(P1)


def make(kind, seed=0, n=400, noise=0.5, outlier_frac=0.3):
    """dict(kp1 [n,2] f32, kp2 [n,2] f32, matches [n,2] i32 identity, n_out planted outliers (the
    first n_out matches), R1, t1, R2, t2)."""
    assert kind in KINDS
    rng = np.random.Generator(np.random.PCG64(seed))
    X = rng.uniform(-2.0, 2.0, size=(n, 3))
    if kind == "plane":
        X[:, 2] = 0.3 * X[:, 0] - 0.2 * X[:, 1]
    R1, t1, R2, t2 = cameras(kind)
    x1, _ = synth.project(R1, t1, F_PX, 0.0, PP[0], PP[1], X)
    x2, _ = synth.project(R2, t2, F_PX, 0.0, PP[0], PP[1], X)
    x1 = x1 + rng.normal(0.0, 1.0, size=x1.shape) * noise
    x2 = x2 + rng.normal(0.0, 1.0, size=x2.shape) * noise
    n_out = int(round(outlier_frac * n))
    x2[:n_out] = rng.uniform(0.0, 1.0, size=(n_out, 2)) * np.array([W, H])
    idx = np.arange(n, dtype=np.int32)
    return dict(kp1=x1.astype(np.float32), kp2=x2.astype(np.float32),
                matches=np.stack([idx, idx], axis=1), n_out=n_out, R1=R1, t1=t1, R2=R2, t2=t2)
