"""GPU parity: next-view registration (sfm_register_batch) vs oracle/sfm_oracle_reg.c.

RANSAC part bit-identical: the winning hypothesis (4h + root), its inlier count and mask.
Refined pose: within 1e-9 (rotation matrix entries) / 1e-9 relative (t) of the numpy
Gauss-Newton restatement (oracle/recon.py reg_refine).  Batch-composition invariance: an image
registered alone or inside a batch gives identical results.
"""
import numpy as np
import pytest

import oracle as O
import recon
import sfmcore

pytestmark = pytest.mark.gpu


def _image(rng, n, outlier_frac=0.4, k1=0.02):
    from scipy.spatial.transform import Rotation
    R = Rotation.random(random_state=int(rng.integers(1 << 30))).as_matrix()
    X = rng.uniform(-2, 2, size=(n, 3))
    t = rng.normal(size=3)
    t = t + np.array([0, 0, 8 - (X @ R.T + t)[:, 2].min()])
    intr = np.array([1000.0, k1, 960.0, 540.0])
    P = X @ R.T + t
    q = P[:, :2] / P[:, 2:]
    xy = intr[0] * (1 + intr[1] * (q * q).sum(1, keepdims=True)) * q + intr[2:]
    xy += rng.normal(0, 0.5, size=xy.shape)
    out = rng.random(n) < outlier_frac
    xy[out] = rng.uniform([0, 0], [1920, 1080], size=(int(out.sum()), 2))
    return dict(R=R, t=t, X=X, xy=xy, intr=intr)


def _gpu(images, ids, n_hyp=512, thr=3.0, refine=True):
    import torch
    ptr = np.r_[0, np.cumsum([len(im["xy"]) for im in images])].astype(np.int32)
    cat = lambda k: np.concatenate([im[k] for im in images]) if images else np.zeros((0, 3))
    T = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    cams, cnt, key, mask = sfmcore.context(0).register_batch(
        T(ptr, np.int32), T(cat("xy"), np.float64), T(cat("X"), np.float64),
        T(np.stack([im["intr"] for im in images]), np.float64), T(ids, np.int32), n_hyp=n_hyp,
        thr=thr, seed=42, refine=refine)
    return cams.cpu().numpy(), cnt.cpu().numpy(), key.cpu().numpy(), mask.cpu().numpy(), ptr


def test_register_matches_oracle_bitwise():
    rng = np.random.default_rng(0)
    # sizes around the scoring kernel's correspondence slices (REG_SPLIT 4): 3 and 5 leave empty
    # or one-correspondence slices, 1000 is many per slice
    images = [_image(rng, n) for n in (300, 50, 1000, 7, 3, 5)]
    ids = np.array([3, 11, 5, 8, 2, 9], np.int32)
    cams, cnt, key, mask, ptr = _gpu(images, ids)
    for i, im in enumerate(images):
        o = O.reg_ransac(im["xy"], im["X"], im["intr"], img=int(ids[i]), n_hyp=512, seed=42,
                         thr=3.0)
        assert cnt[i] == o["count"] and key[i] == o["key"]
        np.testing.assert_array_equal(mask[ptr[i]:ptr[i + 1]], o["mask"])
        Rr, tr = recon.reg_refine(o["R"], o["t"], im["xy"], im["X"], im["intr"], o["mask"])
        np.testing.assert_allclose(recon._rotmat(cams[i, :3]), Rr, atol=1e-9)
        np.testing.assert_allclose(cams[i, 3:6], tr, rtol=1e-9, atol=1e-9)
        np.testing.assert_array_equal(cams[i, 6:], im["intr"][:2])
        if len(im["xy"]) >= 50:                      # accurate pose after refinement
            np.testing.assert_allclose(Rr, im["R"], atol=2e-3)


def test_register_failures_and_batch_invariance():
    rng = np.random.default_rng(1)
    good = _image(rng, 200)
    tiny = _image(rng, 2)
    cams, cnt, key, mask, _ = _gpu([tiny, good], np.array([0, 1], np.int32))
    assert cnt[0] == -1 and key[0] == -1 and np.all(cams[0] == 0)
    cams1, cnt1, key1, mask1, _ = _gpu([good], np.array([1], np.int32))
    assert cnt1[0] == cnt[1] and key1[0] == key[1]
    np.testing.assert_array_equal(cams1[0], cams[1])
    np.testing.assert_array_equal(mask1, mask[2:])


def _oracle(im, img):
    import recon_edge_cases as E
    return O.reg_ransac(im["xy"], im["X"], im["intr"], img=img, n_hyp=E.REG_N_HYP, seed=E.REG_SEED,
                        thr=E.REG_THR)


def test_register_rotations_at_zero_and_the_half_turn():
    """True rotations I, exp(3e-9 a) and half turns less 1e-8 / 3e-7 about e_x, e_y, e_z and a
    random axis (noise-free inliers, 30 % outliers): the RANSAC part bit-identical, the unrefined
    pose's angle-axis within 1e-12 of the oracle's rotation matrix (50-digit rotmat), the refined
    one within 1e-9 of the numpy Gauss-Newton restatement."""
    import hp_ref
    import recon_edge_cases as E
    images = E.reg_pose_images()
    ids = np.arange(len(images), dtype=np.int32) + 2
    kw = dict(n_hyp=E.REG_N_HYP, thr=E.REG_THR)
    raw, cnt, key, mask, ptr = _gpu(images, ids, refine=False, **kw)
    ref, cnt2, key2, mask2, _ = _gpu(images, ids, refine=True, **kw)
    np.testing.assert_array_equal(cnt, cnt2)
    np.testing.assert_array_equal(key, key2)
    np.testing.assert_array_equal(mask, mask2)
    sines = []
    for i, im in enumerate(images):
        o = _oracle(im, int(ids[i]))
        assert cnt[i] == o["count"] and key[i] == o["key"] and o["count"] >= 100
        np.testing.assert_array_equal(mask[ptr[i]:ptr[i + 1]], o["mask"])
        w = np.array([o["R"][2, 1] - o["R"][1, 2], o["R"][0, 2] - o["R"][2, 0],
                      o["R"][1, 0] - o["R"][0, 1]])
        sines.append(0.5 * np.linalg.norm(w))
        err = hp_ref.rot_err(raw[i, :3], [[hp_ref.mp.mpf(float(x)) for x in row] for row in o["R"]])
        assert err <= E.LOGMAP_TOL, (i, err)
        assert np.linalg.norm(raw[i, :3]) <= np.pi + 1e-12
        np.testing.assert_array_equal(raw[i, 3:6], o["t"])
        np.testing.assert_array_equal(raw[i, 6:], im["intr"][:2])
        Rr, tr = recon.reg_refine(o["R"], o["t"], im["xy"], im["X"], im["intr"], o["mask"])
        np.testing.assert_allclose(recon._rotmat(ref[i, :3]), Rr, atol=1e-9)
        np.testing.assert_allclose(ref[i, 3:6], tr, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(Rr, im["R"], atol=1e-6)
    print("sin(theta) of the RANSAC rotations:", " ".join(f"{s:.1e}" for s in sines))
    assert min(sines) < 1e-7 and max(sines) > 1e-7       # both sides of the near-0 / near-pi switch


def test_register_degenerate_and_small_inside_a_batch():
    """Collinear and coincident 3-D points (n >= 3 but no valid hypothesis), planar structure,
    n = 3 and n = 4, between good images of one batch: counts, keys and masks as the oracle's,
    failures zeroed, and the good images as when registered alone."""
    import recon_edge_cases as E
    kinds, images = zip(*E.reg_degenerate_images())
    ids = np.arange(len(images), dtype=np.int32) + 1
    kw = dict(n_hyp=E.REG_N_HYP, thr=E.REG_THR)
    cams, cnt, key, mask, ptr = _gpu(list(images), ids, **kw)
    for i, (kind, im) in enumerate(zip(kinds, images)):
        o = _oracle(im, int(ids[i]))
        assert cnt[i] == o["count"] and key[i] == o["key"], (kind, cnt[i], key[i], o)
        m = mask[ptr[i]:ptr[i + 1]]
        if kind in ("collinear", "coincident"):
            assert cnt[i] == -1 and key[i] == -1 and np.all(cams[i] == 0) and not m.any()
            continue
        np.testing.assert_array_equal(m, o["mask"])
        assert cnt[i] >= min(len(im["xy"]), 50) * 0.6, (kind, cnt[i])
        Rr, tr = recon.reg_refine(o["R"], o["t"], im["xy"], im["X"], im["intr"], o["mask"])
        np.testing.assert_allclose(recon._rotmat(cams[i, :3]), Rr, atol=1e-9)
        np.testing.assert_allclose(cams[i, 3:6], tr, rtol=1e-9, atol=1e-9)
    good = [i for i, k in enumerate(kinds) if k == "good"]
    alone = _gpu([images[i] for i in good], ids[good], **kw)
    np.testing.assert_array_equal(alone[0], cams[good])
    np.testing.assert_array_equal(alone[1], cnt[good])
    np.testing.assert_array_equal(alone[2], key[good])
    np.testing.assert_array_equal(alone[3], np.concatenate([mask[ptr[i]:ptr[i + 1]] for i in good]))
