"""ctypes front-end of tests/tri_ref.c, the CPU statement of the robust triangulation spec (TEST
INFRASTRUCTURE ONLY; the product package never imports it).  Builds tests/lib/libtriref.so on
demand with the oracle Makefile's numerics flags (those of tests/pose_ref.py)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "tri_ref.c")
_LIB_DIR = os.path.join(_HERE, "lib")
_LIB_PATH = os.path.join(_LIB_DIR, "libtriref.so")
CFLAGS = ["-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-fPIC"]
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
        vp, i32, f64, u64, u32 = C.c_void_p, C.c_int32, C.c_double, C.c_uint64, C.c_uint32
        L.triref_n_hyp.argtypes = [i32, i32]
        L.triref_n_hyp.restype = i32
        L.triref_pair.argtypes = [i32, i32, i32, u64, u32, vp]
        L.triref_pair.restype = None
        L.triref_cam_table.argtypes = [i32, vp, vp, vp]
        L.triref_cam_table.restype = None
        L.triref_run.argtypes = [vp, i32, vp, vp, vp, vp, f64, f64, i32, u64, vp, vp, vp, vp]
        L.triref_run.restype = None
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def max_cos2(min_angle_deg: float) -> float:
    """cos^2 of the angle gate, as the library's host side computes it."""
    return float(np.cos(np.deg2rad(float(min_angle_deg))) ** 2)


def n_hyp(n: int, max_hyp: int) -> int:
    return int(lib().triref_n_hyp(int(n), int(max_hyp)))


def pair(h: int, n: int, max_hyp: int, seed: int, pt_id: int):
    ij = np.zeros(2, np.int32)
    lib().triref_pair(int(h), int(n), int(max_hyp), int(seed), int(pt_id) & 0xFFFFFFFF, _p(ij))
    return int(ij[0]), int(ij[1])


def cam_table(cams, pp) -> np.ndarray:
    """[n_cam, 20] per-camera table with libm's sin / cos."""
    cams = np.ascontiguousarray(cams, np.float64).reshape(-1, 8)
    pp = np.ascontiguousarray(pp, np.float64).reshape(-1, 2)
    tab = np.zeros((len(cams), 20), np.float64)
    lib().triref_cam_table(len(cams), _p(cams), _p(pp), _p(tab))
    return tab


def run(tab, pt_ptr, cam_idx, uv, pt_id, thr=4.0, min_angle_deg=1.0, max_hyp=64, seed=42):
    """The batch from a camera table [n_cam, 20]: (pts [n,3], stats [n,4], mask [n_obs] u8, info
    [n,2] i32) as Context.triangulate_robust returns them."""
    tab = np.ascontiguousarray(tab, np.float64)
    pt_ptr = np.ascontiguousarray(pt_ptr, np.int32)
    cam_idx = np.ascontiguousarray(cam_idx, np.int32)
    uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
    pt_id = np.ascontiguousarray(pt_id, np.int32)
    n = len(pt_ptr) - 1
    pts, stats = np.zeros((n, 3)), np.zeros((n, 4))
    mask, info = np.zeros(len(cam_idx), np.uint8), np.zeros((n, 2), np.int32)
    if n > 0:
        lib().triref_run(_p(tab), n, _p(pt_ptr), _p(cam_idx), _p(uv), _p(pt_id), float(thr),
                         max_cos2(min_angle_deg), int(max_hyp), int(seed), _p(pts), _p(stats),
                         _p(mask), _p(info))
    return pts, stats, mask, info
