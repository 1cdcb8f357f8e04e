"""ctypes front-end of tests/h_ref.c, the CPU restatement of the homography RANSAC spec (TEST
INFRASTRUCTURE ONLY; the product package never imports it).  Builds tests/lib/libhref.so on demand
with the oracle Makefile's numerics flags."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "h_ref.c")
_LIB_DIR = os.path.join(_HERE, "lib")
_LIB_PATH = os.path.join(_LIB_DIR, "libhref.so")
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
        vp, i32, u32, u64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64
        L.href_philox4x32_10.argtypes = [vp, vp, vp]
        L.href_sample4.argtypes = [u64, u32, u32, u32, i32, vp]
        L.href_normalize.argtypes = [vp, i32, vp, vp, vp, vp]
        L.href_fit_h4.argtypes = [vp, vp, vp, vp]
        L.href_fit_h4.restype = i32
        L.href_ransac_h.argtypes = [vp, vp, i32, i32, u64, u32, u32, C.c_float, vp, vp, vp, vp,
                                    vp, vp]
        L.href_ransac_h.restype = i32
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def philox(ctr, key):
    c, k = np.asarray(ctr, np.uint32), np.asarray(key, np.uint32)
    o = np.zeros(4, np.uint32)
    lib().href_philox4x32_10(_p(c), _p(k), _p(o))
    return o


def sample4(seed, pa, pb, h, M):
    o = np.zeros(4, np.int32)
    lib().href_sample4(seed, pa, pb, h, M, _p(o))
    return o


def normalize(xy):
    xy = np.ascontiguousarray(xy, np.float32)
    out = np.zeros_like(xy)
    cx, cy, s = C.c_float(), C.c_float(), C.c_float()
    lib().href_normalize(_p(xy), xy.shape[0], _p(out), C.byref(cx), C.byref(cy), C.byref(s))
    return out, cx.value, cy.value, s.value


def fit_h4(p1, p2):
    """(valid, H [9] f32, sign) from 4 normalised correspondences."""
    p1 = np.ascontiguousarray(p1, np.float32)
    p2 = np.ascontiguousarray(p2, np.float32)
    H = np.zeros(9, np.float32)
    sgn = C.c_int32()
    ok = lib().href_fit_h4(_p(p1), _p(p2), _p(H), C.byref(sgn))
    return bool(ok), H, sgn.value


def ransac_h(xy1, xy2, H=4096, seed=42, pa=0, pb=1, thr=4.0, per_hyp=False):
    """dict(count, best_h, H (normalised, 9), norm (6), mask (u8 [M])); with per_hyp also counts
    [H] i32 (-1 invalid) and hyp_H [H, 9] f32 (zero if invalid)."""
    xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2)
    xy2 = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
    M = xy1.shape[0]
    bh = np.zeros(1, np.int32)
    Hn = np.zeros(9, np.float32)
    nrm = np.zeros(6, np.float32)
    mask = np.zeros(max(M, 1), np.uint8)
    counts = np.zeros(H, np.int32) if per_hyp else None
    hyp_H = np.zeros((H, 9), np.float32) if per_hyp else None
    c = lib().href_ransac_h(_p(xy1), _p(xy2), M, H, seed, pa, pb, thr, _p(bh), _p(Hn), _p(nrm),
                            _p(mask), _p(counts) if per_hyp else None,
                            _p(hyp_H) if per_hyp else None)
    r = dict(count=c, best_h=int(bh[0]), H=Hn, norm=nrm, mask=mask[:M])
    if per_hyp:
        r.update(counts=counts, hyp_H=hyp_H)
    return r
