"""ctypes front-end of tests/guided_ref.c, the CPU statement of the guided-matching spec (TEST
INFRASTRUCTURE ONLY; the product package never imports it).  Builds tests/lib/libguidedref.so on
demand with the oracle Makefile's numerics flags (those of tests/tri_ref.py)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "guided_ref.c")
_LIB_DIR = os.path.join(_HERE, "lib")
_LIB_PATH = os.path.join(_LIB_DIR, "libguidedref.so")
CFLAGS = ["-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-fPIC"]
XC_NONE, XC_MUTUAL = 0, 1
_lib = None


def build(force: bool = False) -> str:
    stale = not os.path.exists(_LIB_PATH) or os.path.getmtime(_LIB_PATH) < os.path.getmtime(_SRC)
    if force or stale:
        os.makedirs(_LIB_DIR, exist_ok=True)
        tmp = _LIB_PATH + f".tmp{os.getpid()}"
        subprocess.run(["gcc", *CFLAGS, "-shared", "-o", tmp, _SRC, "-lm"], check=True)
        os.replace(tmp, _LIB_PATH)
    return _LIB_PATH


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
        L.guidedref_cand.argtypes = [vp, vp, f32, vp, vp, i32, vp]
        L.guidedref_cand.restype = None
        L.guidedref_batch.argtypes = [vp, vp, vp, i32, i32, vp, i32, vp, vp, vp, i32, i32, i32,
                                      i32, f32, i64, vp, vp, vp, vp]
        L.guidedref_batch.restype = None
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def cand(F, norm, thr, xy1, xy2) -> np.ndarray:
    """cand of the point pairs (xy1[m], xy2[m]) in pixels under (F [9], norm [6], thr): u8 [n]."""
    F = np.ascontiguousarray(F, np.float32).reshape(9)
    norm = np.ascontiguousarray(norm, np.float32).reshape(6)
    xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2)
    xy2 = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
    out = np.zeros(len(xy1), np.uint8)
    if len(xy1):
        lib().guidedref_cand(_p(F), _p(norm), float(thr), _p(xy1), _p(xy2), len(xy1), _p(out))
    return out


def batch(desc, n_kp, kps, pairs, inl_count, F, norm, thr=4.0, ratio=(4, 5),
          cross_check=XC_MUTUAL, max_dist=128450, min_inliers=15):
    """The batch as Context.guided_match_batch(..., with_ncand=True) returns it: (count [P],
    match [P,k_max,2], dist [P,k_max], ncand [P,k_max]) int32, rows zero from count on."""
    desc = np.ascontiguousarray(desc, np.uint8)
    n_img, k_max, dim = desc.shape
    assert dim == 128
    n_kp = np.ascontiguousarray(n_kp, np.int32)
    kps = np.ascontiguousarray(kps, np.float32).reshape(n_img, k_max, 2)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    P = len(pairs)
    inl_count = np.ascontiguousarray(inl_count, np.int32).reshape(P)
    F = np.ascontiguousarray(F, np.float32).reshape(P, 9)
    norm = np.ascontiguousarray(norm, np.float32).reshape(P, 6)
    count = np.zeros(P, np.int32)
    match = np.zeros((P, k_max, 2), np.int32)
    dist = np.zeros((P, k_max), np.int32)
    ncand = np.zeros((P, k_max), np.int32)
    num, den = (0, 0) if ratio is None else ratio
    if P:
        lib().guidedref_batch(_p(desc), _p(n_kp), _p(kps), n_img, k_max, _p(pairs), P,
                              _p(inl_count), _p(F), _p(norm), int(cross_check), int(num),
                              int(den), int(min_inliers), float(thr), int(max_dist), _p(count),
                              _p(match), _p(dist), _p(ncand))
    return count, match, dist, ncand
