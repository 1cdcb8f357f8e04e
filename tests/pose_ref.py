"""ctypes front-end of tests/pose_ref.c, the CPU statement of the two-view relative pose spec (TEST
INFRASTRUCTURE ONLY; the product package never imports it).  Builds tests/lib/libposeref.so on
demand with the oracle Makefile's numerics flags (those of tests/h_ref.py)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "pose_ref.c")
_LIB_DIR = os.path.join(_HERE, "lib")
_LIB_PATH = os.path.join(_LIB_DIR, "libposeref.so")
CFLAGS = ["-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-fPIC"]
_lib = None


def build(force: bool = False) -> str:
    stale = not os.path.exists(_LIB_PATH) or os.path.getmtime(_LIB_PATH) < os.path.getmtime(_SRC)
    if force or stale:
        os.makedirs(_LIB_DIR, exist_ok=True)
        tmp = _LIB_PATH + ".tmp"
        subprocess.run(["gcc", *CFLAGS, "-shared", "-o", tmp, _SRC, "-lm"], check=True)
        os.replace(tmp, _LIB_PATH)
    return _LIB_PATH


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
        L.pref_undistort.argtypes = [f32, f32, vp, vp]
        L.pref_undistort.restype = None
        L.pref_normal_matrix.argtypes = [vp, vp, vp, i32, vp]
        L.pref_normal_matrix.restype = None
        L.pref_pose.argtypes = [vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, vp, vp]
        L.pref_pose.restype = None
        L.pref_candidates.argtypes = [vp, vp, vp, vp]
        L.pref_candidates.restype = i32
        L.pref_pose_batch.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, i32, f32, vp, vp,
                                      vp, vp, vp]
        L.pref_pose_batch.restype = None
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def wide_key(min_angle_deg: float) -> np.float32:
    """The key of a ray angle (below 90 degrees): sin^2, as the library's host side computes it."""
    return np.float32(np.sin(np.deg2rad(float(min_angle_deg))) ** 2)


def key_to_degrees(key) -> np.ndarray:
    """Angle of a key: asin(sqrt(key)) up to 90 degrees (key <= 1), 180 - asin(sqrt(2 - key))
    above."""
    k = np.asarray(key, np.float64)
    lo = np.degrees(np.arcsin(np.sqrt(np.clip(k, 0.0, 1.0))))
    hi = 180.0 - np.degrees(np.arcsin(np.sqrt(np.clip(2.0 - k, 0.0, 1.0))))
    return np.where(k <= 1.0, lo, hi)


def undistort(kp, intr) -> np.ndarray:
    """kp [n,2] f32 pixels, intr (f, k1, cx, cy) -> [n,2] f64 normalised undistorted."""
    kp = np.ascontiguousarray(kp, np.float32).reshape(-1, 2)
    it = np.ascontiguousarray(intr, np.float64)
    out = np.zeros((len(kp), 2), np.float64)
    L = lib()
    for i in range(len(kp)):
        L.pref_undistort(float(kp[i, 0]), float(kp[i, 1]), _p(it), _p(out[i]))
    return out


def normal_matrix(x1, x2, mask=None) -> np.ndarray:
    """N = A^T A [9,9] of the masked-in correspondences, in the spec's summation order."""
    x1 = np.ascontiguousarray(x1, np.float64).reshape(-1, 2)
    x2 = np.ascontiguousarray(x2, np.float64).reshape(-1, 2)
    M = len(x1)
    mk = np.ones(M, np.uint8) if mask is None else np.ascontiguousarray(mask, np.uint8)
    N = np.zeros(81, np.float64)
    lib().pref_normal_matrix(_p(x1), _p(x2), _p(mk), M, _p(N))
    return N.reshape(9, 9)


def candidates(E):
    """(Ra [9], Rb [9], u3 [3], ok) of a fitted E [9]: candidate c is (Rb if c >> 1 else Ra,
    -u3 if c & 1 else u3); ok is False where the pose reports status 2."""
    E = np.ascontiguousarray(E, np.float64).ravel()
    Ra, Rb, u3 = np.zeros(9), np.zeros(9), np.zeros(3)
    ok = lib().pref_candidates(_p(E), _p(Ra), _p(Rb), _p(u3))
    return Ra, Rb, u3, bool(ok)


def _result(E, R, t, stat, med):
    return dict(E=E, R=R, t=t, stat=stat, median_key=med)


def pose(x1, x2, mask=None, inl_count=None, min_inliers=15, min_angle_deg=2.0):
    """One pair from undistorted coordinates x1 / x2 [M,2] f64.  dict(E [9], R [9], t [3],
    stat [8] = (status, best, n_front[4], n_wide, inliers used), median_key f32)."""
    x1 = np.ascontiguousarray(x1, np.float64).reshape(-1, 2)
    x2 = np.ascontiguousarray(x2, np.float64).reshape(-1, 2)
    M = len(x1)
    mk = np.ones(max(M, 1), np.uint8) if mask is None else np.ascontiguousarray(mask, np.uint8)
    ic = int(mk[:M].sum()) if inl_count is None else int(inl_count)
    E, R, t = np.zeros(9), np.zeros(9), np.zeros(3)
    stat, med = np.zeros(8, np.int32), np.zeros(1, np.float32)
    lib().pref_pose(_p(x1), _p(x2), _p(mk), M, ic, int(min_inliers),
                    float(wide_key(min_angle_deg)), _p(E), _p(R), _p(t), _p(stat), _p(med))
    return _result(E, R, t, stat, med[0])


def pose_batch(kps, intr, pairs, count, match, mask, inl_count, min_inliers=15,
               min_angle_deg=2.0):
    """The batch on host arrays shaped like Context.two_view_pose_batch's device tensors.
    dict(E [P,9], R [P,9], t [P,3], stat [P,8], median_key [P])."""
    kps = np.ascontiguousarray(kps, np.float32)
    intr = np.ascontiguousarray(intr, np.float64)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    count = np.ascontiguousarray(count, np.int32)
    match = np.ascontiguousarray(match, np.int32)
    mask = np.ascontiguousarray(mask, np.uint8)
    inl_count = np.ascontiguousarray(inl_count, np.int32)
    n_img, k_max, _ = kps.shape
    P = len(pairs)
    E, R, t = np.zeros((P, 9)), np.zeros((P, 9)), np.zeros((P, 3))
    stat, med = np.zeros((P, 8), np.int32), np.zeros(P, np.float32)
    if P:
        lib().pref_pose_batch(_p(kps), n_img, k_max, _p(pairs), P, _p(count), _p(match), _p(mask),
                              _p(inl_count), _p(intr), int(min_inliers),
                              float(wide_key(min_angle_deg)), _p(E), _p(R), _p(t), _p(stat),
                              _p(med))
    return _result(E, R, t, stat, med)
