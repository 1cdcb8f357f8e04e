"""Shared inputs of the guided-matching tests (tests/test_guided_ref_cpu.py, tests/test_gpu_guided.py).

make_case(k_max): 6 images in a SIZE x SIZE pixel frame, every ordered pair plus one (a, a), and a
supplied (not estimated) two-view geometry per pair: a rank-2 F from a random relative pose,
expressed in a random Hartley-like normalisation (centres near the frame's middle, scales in
0.002 .. 0.02), and inl_count above the bar.  The keypoints are uniform in the frame, so at
THR = 9 px^2 a query's band (6 px wide, up to ~600 px long) holds about 1 % of the other image's
keypoints: rows with 0, 1, 2 and many candidates all occur, and a few candidates per row on
average where the other image is full (asserted in test_guided_ref_cpu.py).  The descriptors come from a small pool of bases with sparse
noise and some exact copies, so near ties and exact ties are frequent.

The image sizes of the two cases together hold 0, 1, 2, 31, 32, 33, 127, 128, 129 and both k_max:
130 crosses the 128-row groups, 520 the 512-query workgroup.
"""
from __future__ import annotations

import numpy as np

SIZE = 600.0
THR = 9.0
N_KP = {130: [130, 0, 1, 32, 127, 129], 520: [520, 2, 31, 33, 128, 513]}
# the four rule combinations of the case-set test: (cross_check, ratio, max_dist)
RULES = {"none": (0, None, -1), "ratio": (0, (4, 5), -1), "mutual": (1, None, -1),
         "mutual_ratio_cap": (1, (4, 5), 60000)}


def _rot(rng, max_deg):
    w = rng.normal(size=3)
    w /= np.linalg.norm(w)
    th = np.deg2rad(rng.uniform(-max_deg, max_deg))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pair_geometry(rng):
    """(F [9] f32 normalised, norm [6] f32) of one random relative pose."""
    f = 500.0
    Kc = np.array([[f, 0, SIZE / 2], [0, f, SIZE / 2], [0, 0, 1.0]])
    R = _rot(rng, 20.0)
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(Kc)
    Fpix = Ki.T @ tx @ R @ Ki
    norm = np.array([SIZE / 2 + rng.uniform(-40, 40), SIZE / 2 + rng.uniform(-40, 40),
                     np.exp(rng.uniform(np.log(0.002), np.log(0.02))),
                     SIZE / 2 + rng.uniform(-40, 40), SIZE / 2 + rng.uniform(-40, 40),
                     np.exp(rng.uniform(np.log(0.002), np.log(0.02)))], np.float32)
    cx1, cy1, s1, cx2, cy2, s2 = [float(v) for v in norm]
    T1i = np.array([[1 / s1, 0, cx1], [0, 1 / s1, cy1], [0, 0, 1.0]])
    T2i = np.array([[1 / s2, 0, cx2], [0, 1 / s2, cy2], [0, 0, 1.0]])
    Fn = T2i.T @ Fpix @ T1i          # F_pix = T2^T Fn T1
    Fn /= np.linalg.norm(Fn)
    return Fn.reshape(9).astype(np.float32), norm


def descriptors(rng, n, n_base=24):
    base = rng.integers(0, 256, size=(n_base, 128))
    d = base[rng.integers(0, n_base, size=n)].copy()
    noisy = rng.random(n) < 0.85          # the rest are exact copies of their base
    for i in np.nonzero(noisy)[0]:
        dims = rng.choice(128, size=int(rng.integers(1, 6)), replace=False)
        d[i, dims] += rng.integers(-40, 41, size=len(dims))
    return np.clip(d, 0, 255).astype(np.uint8)


def make_case(k_max: int, seed: int = 7) -> dict:
    rng = np.random.Generator(np.random.PCG64([seed, k_max]))
    n_kp = np.array(N_KP[k_max], np.int32)
    n_img = len(n_kp)
    desc = descriptors(rng, n_img * k_max).reshape(n_img, k_max, 128)
    kps = rng.uniform(0.0, SIZE, size=(n_img, k_max, 2)).astype(np.float32)
    pairs = [(a, b) for a in range(n_img) for b in range(n_img) if a != b] + [(0, 0)]
    pairs = np.array(pairs, np.int32)
    geo = [pair_geometry(rng) for _ in pairs]
    F = np.stack([g[0] for g in geo])
    norm = np.stack([g[1] for g in geo])
    inl_count = np.full(len(pairs), 100, np.int32)
    return dict(desc=desc, kps=kps, n_kp=n_kp, pairs=pairs, F=F, norm=norm, inl_count=inl_count,
                k_max=k_max, thr=THR)


HORIZONTAL_F = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)


def all_candidates_case(k_max: int, n_kp, seed: int = 11) -> dict:
    """Every (i, j) is a candidate: the horizontal-epipolar F, every keypoint on one y, equal
    norms.  The guided result is then the plain match of the descriptors."""
    rng = np.random.Generator(np.random.PCG64([seed, k_max]))
    n_kp = np.array(n_kp, np.int32)
    n_img = len(n_kp)
    desc = descriptors(rng, n_img * k_max).reshape(n_img, k_max, 128)
    kps = np.zeros((n_img, k_max, 2), np.float32)
    kps[..., 0] = rng.uniform(0.0, SIZE, size=(n_img, k_max))
    kps[..., 1] = 250.0
    pairs = np.array([(a, b) for a in range(n_img) for b in range(n_img) if a != b], np.int32)
    P = len(pairs)
    norm = np.tile(np.array([300, 250, 0.01, 300, 250, 0.01], np.float32), (P, 1))
    return dict(desc=desc, kps=kps, n_kp=n_kp, pairs=pairs, F=np.tile(HORIZONTAL_F, (P, 1)),
                norm=norm, inl_count=np.full(P, 100, np.int32), k_max=k_max, thr=4.0)
