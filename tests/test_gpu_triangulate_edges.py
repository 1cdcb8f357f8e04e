"""GPU: sfm_triangulate against the 50-digit reference (tests/hp_ref.py) on the edge cases of
tests/recon_edge_cases.py: ray angles from 30 down to 0.05 degrees, ragged track lengths up to 150
with 0- and 1-observation tracks between them, statuses 2 and 3, both rotmat branches, n_pt 0 and 1,
and bitwise invariance to the batch a point is in.

Points within K eps kappa (1 + |X_ref|^2) with kappa from the reference's eigenvalues, statistics
within the tolerance propagated from that, statuses equal for every point (recon_edge_cases.py
derives K and states why the comparison of statuses is fair).
"""
import numpy as np
import pytest

import recon_edge_cases as E
import sfmcore

pytestmark = pytest.mark.gpu


def _gpu(case, sel=None):
    """ctx.triangulate of the case, or of its points sel (in that order) as a batch of their own."""
    import torch
    ptr, ci, uv = case["pt_ptr"], case["cam_idx"], case["uv"]
    if sel is not None:
        obs = np.concatenate([np.arange(ptr[p], ptr[p + 1]) for p in sel] + [np.zeros(0, int)])
        obs = obs.astype(np.int64)
        ptr = np.r_[0, np.cumsum([ptr[p + 1] - ptr[p] for p in sel])].astype(np.int32)
        ci, uv = ci[obs], uv[obs]
    assert ptr[-1] == len(ci) == len(uv) and (len(ci) == 0 or 0 <= ci.min() <= ci.max() < len(case["cams"]))
    T = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    pts, st = sfmcore.context(0).triangulate(
        T(case["cams"], np.float64), T(case["pp"], np.float64), T(ptr, np.int32), T(ci, np.int32),
        T(uv.reshape(-1, 2), np.float64))
    return pts.cpu().numpy(), st.cpu().numpy()


@pytest.fixture(scope="module")
def narrow_gpu():
    return _gpu(E.tri_case("narrow"))


def test_narrow_baselines(narrow_gpu):
    E.check_triangulation("narrow", *narrow_gpu)


@pytest.mark.parametrize("name", ["ragged", "rotmat", "single"])
def test_case_matches_50_digits(name):
    E.check_triangulation(name, *_gpu(E.tri_case(name)))


def test_statuses_2_and_3():
    pts, st = _gpu(E.tri_case("status"))
    assert tuple(st[:, 3].astype(int)) == E.STATUS_EXPECTED
    assert np.all(pts[[0, 2]] == 0.0) and np.all(st[[0, 2], :3] == 0.0)   # at infinity: zeros
    assert pts[1, 0] != 0.0 and pts[1, 2] < 0.0 and st[1, 2] < 0.0        # behind: still written
    E.check_triangulation("status", pts, st)


def test_no_points_returns_empty():
    case = E.tri_case("single")
    pts, st = _gpu(case, sel=[])
    assert pts.shape == (0, 3) and st.shape == (0, 4)


def test_point_alone_and_permuted_give_the_same_bytes(narrow_gpu):
    case = E.tri_case("narrow")
    pts, st = narrow_gpu
    for p in (0, 131, 319):                       # a 30, a 1 and a 0.05 degree point
        p1, s1 = _gpu(case, sel=[p])
        assert p1.tobytes() == pts[p:p + 1].tobytes() and s1.tobytes() == st[p:p + 1].tobytes()
    perm = np.random.default_rng(0).permutation(len(pts))
    pp_, sp = _gpu(case, sel=perm)
    assert pp_.tobytes() == pts[perm].tobytes() and sp.tobytes() == st[perm].tobytes()
    E.check_triangulation("narrow", pp_, sp, sel=perm)
