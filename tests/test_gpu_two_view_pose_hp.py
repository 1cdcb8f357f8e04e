"""GPU: the two-view pose batch (sfm_two_view_pose_batch) on the cases of tests/pose_hp_cases.py,
one batch per family: every byte against tests/pose_ref.c, the shape batches included (M at the
256-stride of both kernels, k_max 1 / 8 / 8192, counts and ids outside their arrays), and the
kernels' own outputs against the 50-digit references of tests/hp_ref.py with the tolerances of
test_two_view_pose_hp_cpu.py.  References are cached per process."""
import numpy as np
import pytest

import pose_hp_cases as pc
import pose_ref

pytestmark = pytest.mark.gpu

KEYS = ("E", "R", "t", "stat", "median_key")
BATCHES = {label: (ns, deg) for label, ns, deg in pc.batches()}
WHERE = {n: (label, p) for label, (ns, _) in BATCHES.items() for p, n in enumerate(ns)}
_GOT = {}


def run_pose(ctx, args, **kw):
    import torch
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
    out = ctx.two_view_pose_batch(*dev, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def family(ctx, label):
    if label not in _GOT:
        ns, deg = BATCHES[label]
        _GOT[label] = run_pose(ctx, pc.batch_args(ns), min_inliers=8, min_angle_deg=deg)
    return _GOT[label]


def assert_same_bytes(got, want, what):
    for k in KEYS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        np.testing.assert_array_equal(g.view(np.uint8), w.view(np.uint8), err_msg=f"{what} {k}")


@pytest.mark.parametrize("label", list(BATCHES))
def test_family_byte_parity(ctx, label):
    ns, deg = BATCHES[label]
    want = pose_ref.pose_batch(*pc.batch_args(ns), min_inliers=8, min_angle_deg=deg)
    assert_same_bytes(family(ctx, label), want, label)


@pytest.mark.parametrize("name", pc.names())
def test_kernel_against_50_digits(ctx, name):
    label, p = WHERE[name]
    pc.check(name, pc.row(family(ctx, label), p), "MI355X")


@pytest.mark.parametrize("label", ["stride", "kmax1", "kmax8", "kmax8192", "clamps"])
def test_shape_byte_parity(ctx, label):
    args = pc.shape_batches()[label]
    got = run_pose(ctx, args, min_inliers=8)
    assert_same_bytes(got, pose_ref.pose_batch(*args, min_inliers=8), label)
    if label == "clamps":   # the rule itself: the batch with every id and count clamped beforehand
        assert_same_bytes(got, pose_ref.pose_batch(*pc.clamped(args), min_inliers=8), "clamped")
