"""CPU: the guided-matching spec (tests/guided_ref.c) against the oracle, and the host-side argument
checks of sfm_guided_match_batch.

* With every (i, j) a candidate the reference is oracle.match on the descriptors.
* The reference's cand on the endpoints of oracle.ransac_f's tentative matches is that call's
  inlier mask byte for byte: the coordinate rule and the op sequence are K2's.
* The case set of tests/guided_cases.py has the band statistics the GPU test relies on.
"""
import ctypes as C

import numpy as np
import pytest

import guided_cases as GC
import guided_ref
import oracle
import sfmcore
import synth


def _run(case, **kw):
    return guided_ref.batch(case["desc"], case["n_kp"], case["kps"], case["pairs"],
                            case["inl_count"], case["F"], case["norm"], thr=case["thr"], **kw)


@pytest.mark.parametrize("xc,ratio,max_dist", [(0, None, -1), (0, (4, 5), -1), (1, (4, 5), -1),
                                                (0, None, 30000), (0, (4, 5), 30000),
                                                (1, (4, 5), 30000)])
def test_all_candidates_is_plain_matching(xc, ratio, max_dist):
    case = GC.all_candidates_case(140, [140, 3, 129, 0])
    count, match, dist, ncand = _run(case, cross_check=xc, ratio=ratio, max_dist=max_dist)
    n_kp = case["n_kp"]
    some = 0
    for p, (a, b) in enumerate(case["pairs"]):
        q, t, d = oracle.match(case["desc"][a, :n_kp[a]], case["desc"][b, :n_kp[b]], metric=0,
                               cross_check=xc, ratio=ratio, max_dist=max_dist)
        assert count[p] == len(q)
        np.testing.assert_array_equal(match[p, :len(q), 0], q)
        np.testing.assert_array_equal(match[p, :len(q), 1], t)
        np.testing.assert_array_equal(dist[p, :len(q)], d)
        want = n_kp[b] if n_kp[a] and n_kp[b] else 0
        np.testing.assert_array_equal(ncand[p, :n_kp[a]], want)
        np.testing.assert_array_equal(ncand[p, n_kp[a]:], 0)
        some += len(q)
    assert some >= 20       # the comparison is not vacuous


@pytest.mark.parametrize("seed,thr", [(3, 1.0), (4, 1.0), (5, 4.0)])
def test_cand_is_k2s_inlier_test(seed, thr):
    scene = synth.make_scene(4, 512, seed)
    a, b = 1, 2
    q, t, _ = oracle.match(scene["desc"][a], scene["desc"][b], metric=0, cross_check=1,
                           ratio=(4, 5))
    xy1, xy2 = scene["kps"][a][q], scene["kps"][b][t]
    rs = oracle.ransac_f(xy1, xy2, H=1024, seed=42, pa=a, pb=b, thr=thr)
    assert 20 < rs["count"] < len(q)
    got = guided_ref.cand(rs["F"], rs["norm"], thr, xy1, xy2)
    np.testing.assert_array_equal(got, rs["mask"])


@pytest.mark.parametrize("k_max", [130, 520])
def test_case_set_statistics(k_max):
    case = GC.make_case(k_max)
    assert sorted(set(GC.N_KP[130]) | set(GC.N_KP[520])) == [0, 1, 2, 31, 32, 33, 127, 128, 129,
                                                              130, 513, 520]
    count, _, _, ncand = _run(case, cross_check=0, ratio=None, max_dist=-1)
    Ka = case["n_kp"][case["pairs"][:, 0]]
    Kb = case["n_kp"][case["pairs"][:, 1]]
    rows = np.concatenate([ncand[p, :Ka[p]] for p in range(len(Ka))])
    for n in (0, 1, 2):
        assert (rows == n).sum() > 50
    assert (rows >= 8).sum() >= 3                       # "many"
    full = np.concatenate([ncand[p, :Ka[p]] for p in range(len(Ka)) if Kb[p] == k_max])
    assert 1.0 < full.mean() < 10.0                     # a few candidates per row
    # every rule combination keeps some matches and drops some
    base = int(count.sum())
    for xc, ratio, md in GC.RULES.values():
        c = int(_run(case, cross_check=xc, ratio=ratio, max_dist=md)[0].sum())
        assert 0 < c <= base
        assert c < base or (xc, ratio, md) == GC.RULES["none"]


def test_skip_rule_and_nan():
    case = GC.make_case(130)
    case["inl_count"][2] = 14          # below min_inliers = 15
    case["inl_count"][3] = 7           # below 8 whatever min_inliers
    case["norm"][4, 2] = 0.0
    case["norm"][20, 5] = 0.0
    case["F"][24, 4] = np.nan
    ref = _run(GC.make_case(130), cross_check=1, ratio=(4, 5), max_dist=-1)
    got = _run(case, cross_check=1, ratio=(4, 5), max_dist=-1)
    for p in (2, 3, 4, 20, 24):
        assert ref[0][p] > 0 and got[0][p] == 0 and not got[3][p].any()
    keep = np.setdiff1d(np.arange(len(case["pairs"])), [2, 3, 4, 20, 24])
    for r, g in zip(ref, got):
        np.testing.assert_array_equal(r[keep], g[keep])


# ---- the C-ABI's host side ----------------------------------------------------------------------

def _call(prm, ctx=None, dim=128, k_max=64, arrays=None):
    lib = sfmcore.load_library()
    a = arrays
    return lib.sfm_guided_match_batch(ctx, a, a, a, 2, k_max, dim, a, 1, a, a, a,
                                      C.byref(prm) if prm is not None else None, a, a, a, None)


def _prm(**kw):
    f = dict(struct_size=C.sizeof(sfmcore.GuidedParams), cross_check=1, ratio_num=4, ratio_den=5,
             min_inliers=15, thr=4.0, max_dist=128450)
    f.update(kw)
    return sfmcore.GuidedParams(**f)


def test_library_exports_the_entry_point():
    lib = sfmcore.load_library()
    assert hasattr(lib, "sfm_guided_match_batch")
    assert "sfm_guided_match_batch" in sfmcore.EXPORTED
    assert lib.sfm_version() == 5


def test_argument_checks_without_device():
    lib = sfmcore.load_library()
    err = lambda: lib.sfm_last_error().decode()
    assert _call(None) == -1 and "NULL" in err()
    assert _call(_prm()) == -1 and "ctx is NULL" in err()
    # a non-NULL context pointer is never dereferenced before the array check
    fake = C.c_void_p(C.addressof(C.create_string_buffer(4096)))
    assert _call(_prm(), ctx=fake) == -1 and "NULL array" in err()
    assert _call(_prm(), dim=32) == -1 and "Hamming" in err()
    assert _call(_prm(cross_check=2)) == -1 and "OpenCV" in err()
    assert _call(_prm(thr=0.0)) == -1 and "thr" in err()
    assert _call(_prm(thr=-1.0)) == -1 and "thr" in err()
    assert _call(_prm(thr=float("nan"))) == -1 and "thr" in err()
    assert _call(_prm(struct_size=C.sizeof(sfmcore.GuidedParams) - 4)) == -1
    assert "struct_size" in err()
    assert _call(_prm(), k_max=8193) == -1 and "8192" in err()
