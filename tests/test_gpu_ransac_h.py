"""GPU parity: homography RANSAC (sfm_ransac_h_batch / sfm_ransac_h_counts) against its CPU
restatement tests/h_ref.c, bit for bit: count, winner id, mask, H and norm (every f32 bit), every
hypothesis's count and H, the match-count boundaries (4-match minimum, the F prep's 8, the 16-match
chunk, the prune period), degenerate input, shard invariance, interleaving with the F batch on one
context, and the public layer of geometric_verification."""
import numpy as np
import pytest

import geometric_verification as gv
import h_ref
import two_view_cases as tv

pytestmark = pytest.mark.gpu

_CASES = {}


def case(kind, seed=0):
    if (kind, seed) not in _CASES:
        _CASES[(kind, seed)] = tv.make(kind, seed=seed)
    return _CASES[(kind, seed)]


def batch_of(items):
    """items: list of (image a, image b, kp1, kp2, M).  Identity matches over the first M points.
    Returns numpy (kps [n_img,k_max,2], pairs [P,2], count [P], match [P,k_max,2])."""
    n_img = max(max(a, b) for a, b, *_ in items) + 1
    k_max = max(max(len(k1), len(k2)) for _, _, k1, k2, _ in items)
    kps = np.zeros((n_img, k_max, 2), np.float32)
    for a, b, k1, k2, _ in items:
        kps[a, :len(k1)] = k1
        kps[b, :len(k2)] = k2
    pairs = np.array([[a, b] for a, b, *_ in items], np.int32)
    count = np.array([M for *_, M in items], np.int32)
    match = np.zeros((len(items), k_max, 2), np.int32)
    match[:, :, 0] = match[:, :, 1] = np.arange(k_max)
    return kps, pairs, count, match


def dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def run_h(ctx, items, **kw):
    import torch
    out = ctx.ransac_h_batch(*dev(*batch_of(items)), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_equals_ref(out, p, item, n_hyp, thr, seed=42):
    a, b, k1, k2, M = item
    r = h_ref.ransac_h(k1[:M], k2[:M], H=n_hyp, seed=seed, pa=a, pb=b, thr=thr)
    assert out["inl_count"][p] == r["count"], (p, M)
    assert out["best_h"][p] == r["best_h"], (p, M)
    np.testing.assert_array_equal(out["mask"][p, :M], r["mask"])
    assert not out["mask"][p, M:].any(), "the mask row is zero past the pair's matches"
    np.testing.assert_array_equal(u32(out["H"][p]), u32(r["H"]))
    np.testing.assert_array_equal(u32(out["norm"][p]), u32(r["norm"]))
    return r


# the three kinds under pair ids other than (0, 1): the RNG is keyed by them
def three_kinds(seed=0):
    ids = {"general": (2, 5), "plane": (0, 3), "rot": (4, 1)}
    return [(a, b, case(k, seed)["kp1"], case(k, seed)["kp2"], 400)
            for k, (a, b) in ids.items()]


@pytest.mark.parametrize("n_hyp,thr", [(256, 4.0), (1024, 4.0), (512, 1.0)])
def test_h_bit_exact(ctx, n_hyp, thr):
    items = three_kinds()
    out = run_h(ctx, items, n_hyp=n_hyp, thr=thr)
    for p, it in enumerate(items):
        assert_equals_ref(out, p, it, n_hyp, thr)


def test_h_every_hypothesis(ctx):
    import torch
    items = three_kinds(seed=1)
    args = dev(*batch_of(items))
    counts, norm, hyp_H = ctx.ransac_h_counts(*args, n_hyp=256, thr=4.0, hyp_H=True)
    counts2, _ = ctx.ransac_h_counts(*args, n_hyp=256, thr=4.0)
    out = ctx.ransac_h_batch(*args, n_hyp=256, thr=4.0)
    torch.cuda.synchronize()
    counts, hyp_H = counts.cpu().numpy(), hyp_H.cpu().numpy()
    np.testing.assert_array_equal(counts, counts2.cpu().numpy())
    for p, (a, b, k1, k2, M) in enumerate(items):
        r = h_ref.ransac_h(k1, k2, H=256, seed=42, pa=a, pb=b, thr=4.0, per_hyp=True)
        np.testing.assert_array_equal(counts[p], r["counts"])
        np.testing.assert_array_equal(u32(hyp_H[p]), u32(r["hyp_H"]))
        np.testing.assert_array_equal(u32(norm[p].cpu().numpy()), u32(r["norm"]))
        assert int(out["inl_count"][p]) == counts[p].max()
        assert int(out["best_h"][p]) == int(np.argmax(counts[p]))


BOUNDARY_M = [3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129]


def test_h_match_count_boundaries(ctx):
    c = case("plane")
    items = [(0, 1 + i, c["kp1"], c["kp2"], M) for i, M in enumerate(BOUNDARY_M)]
    out = run_h(ctx, items, n_hyp=256, thr=4.0)
    for p, it in enumerate(items):
        assert_equals_ref(out, p, it, 256, 4.0)
    assert out["inl_count"][0] == -1 and out["best_h"][0] == -1
    assert not out["H"][0].any() and not out["norm"][0].any()
    # and every hypothesis of the small pairs (the sampler's tight ranges, invalid samples)
    import torch
    counts, _, hyp_H = ctx.ransac_h_counts(*dev(*batch_of(items)), n_hyp=256, thr=4.0, hyp_H=True)
    torch.cuda.synchronize()
    counts, hyp_H = counts.cpu().numpy(), hyp_H.cpu().numpy()
    for p, (a, b, k1, k2, M) in enumerate(items):
        r = h_ref.ransac_h(k1[:M], k2[:M], H=256, seed=42, pa=a, pb=b, thr=4.0, per_hyp=True)
        np.testing.assert_array_equal(counts[p], r["counts"])
        np.testing.assert_array_equal(u32(hyp_H[p]), u32(r["hyp_H"]))


def test_h_degenerate_and_empty(ctx):
    rng = np.random.default_rng(0)
    k1 = rng.uniform(0, 1000, size=(64, 2)).astype(np.float32)
    same = np.repeat(k1[:1], 64, axis=0)  # every keypoint of the image identical
    items = [(0, 1, k1, same, 40), (2, 3, same, k1, 40), (4, 5, k1, k1, 0)]
    out = run_h(ctx, items, n_hyp=256, thr=4.0)
    for p, it in enumerate(items):
        assert_equals_ref(out, p, it, 256, 4.0)
    assert out["inl_count"][2] == -1 and out["best_h"][2] == -1


def test_h_norm_equals_f_norm(ctx):
    import torch
    c = case("plane")
    items = three_kinds() + [(0, 6, c["kp1"], c["kp2"], M) for M in (8, 17, 129)]
    args = dev(*batch_of(items))
    oh = ctx.ransac_h_batch(*args, n_hyp=256, thr=4.0)
    of = ctx.ransac_batch(*args, n_hyp=256, thr=1.0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(u32(oh["norm"].cpu().numpy()), u32(of["norm"].cpu().numpy()))


def test_h_shard_invariance(ctx):
    items = three_kinds() + three_kinds(seed=2)
    items = [(a + 10 * (p // 3), b + 10 * (p // 3), k1, k2, M)  # six pairs, twelve images
             for p, (a, b, k1, k2, M) in enumerate(items)]
    both = run_h(ctx, items, n_hyp=512, thr=4.0)
    for p, it in enumerate(items):
        alone = run_h(ctx, [it], n_hyp=512, thr=4.0)
        for k in ("inl_count", "best_h", "mask"):
            np.testing.assert_array_equal(both[k][p], alone[k][0], err_msg=f"{k} pair {p}")
        for k in ("H", "norm"):
            np.testing.assert_array_equal(u32(both[k][p]), u32(alone[k][0]), err_msg=f"{k} pair {p}")


def test_h_interleaved_with_f_on_one_context(ctx):
    import torch
    import sfmcore
    items = three_kinds()
    args = dev(*batch_of(items))
    get = lambda o: {k: v.cpu().numpy() for k, v in o.items()}
    fresh = sfmcore.Context(0)  # a context no F batch ever ran on
    h0 = get(fresh.ransac_h_batch(*args, n_hyp=512, thr=4.0))
    fresh.close()
    f1 = get(ctx.ransac_batch(*args, n_hyp=512, thr=1.0))
    h1 = get(ctx.ransac_h_batch(*args, n_hyp=512, thr=4.0))
    f2 = get(ctx.ransac_batch(*args, n_hyp=512, thr=1.0))
    h2 = get(ctx.ransac_h_batch(*args, n_hyp=512, thr=4.0))
    torch.cuda.synchronize()
    for k in f1:
        assert f1[k].tobytes() == f2[k].tobytes(), k
    for k in h1:
        assert h1[k].tobytes() == h0[k].tobytes(), k
        assert h2[k].tobytes() == h0[k].tobytes(), k
    for p, it in enumerate(items):
        assert_equals_ref(h1, p, it, 512, 4.0)


def test_verify_pair_h(ctx):
    c = case("plane", 1)
    r = h_ref.ransac_h(c["kp1"], c["kp2"], H=512, seed=7, pa=2, pb=9, thr=4.0)
    v = gv.verify_pair_h(c["kp1"], c["kp2"], c["matches"], pair=(2, 9), n_hyp=512, seed=7)
    assert v["count"] == r["count"] and v["best_h"] == r["best_h"] and v["verified"]
    np.testing.assert_array_equal(v["inliers"], np.nonzero(r["mask"])[0])
    np.testing.assert_array_equal(v["H"], gv.denormalize_H(r["H"], r["norm"]))
    few = gv.verify_pair_h(c["kp1"], c["kp2"], c["matches"][:3], n_hyp=256)
    assert few["count"] == 0 and not few["verified"] and few["best_h"] == -1


@pytest.mark.parametrize("kind", tv.KINDS)
def test_two_view_geometry_classes(ctx, kind):
    c = case(kind)
    g = gv.two_view_geometry(c["kp1"], c["kp2"], c["matches"], pair=(0, 1), n_hyp=1024)
    assert g["config"] == ("general" if kind == "general" else "planar_or_panoramic")
    f = gv.verify_pair(c["kp1"], c["kp2"], c["matches"], pair=(0, 1), n_hyp=1024)
    h = gv.verify_pair_h(c["kp1"], c["kp2"], c["matches"], pair=(0, 1), n_hyp=1024)
    assert g["f_count"] == f["count"] and g["h_count"] == h["count"]
    np.testing.assert_array_equal(g["f_inliers"], f["inliers"])
    np.testing.assert_array_equal(g["h_inliers"], h["inliers"])
    np.testing.assert_array_equal(g["F"], f["F"])
    np.testing.assert_array_equal(g["H"], h["H"])
    assert g["h_ratio"] == g["h_count"] / g["f_count"]


class _Pair:
    def __init__(self, a, b, matches):
        self.img_inx_1, self.img_inx_2, self.matches = a, b, matches


def _pair_list():
    kps, prs = {}, []
    for i, kind in enumerate(tv.KINDS):
        c = case(kind)
        kps[2 * i], kps[2 * i + 1] = c["kp1"], c["kp2"]
        prs.append(_Pair(2 * i, 2 * i + 1, [tuple(m) for m in c["matches"]]))
    return prs, [kps[i] for i in range(6)]


def test_verify_pairs_with_homography(ctx):
    prs, kps = _pair_list()
    plain, _ = _pair_list()
    got = gv.verify_pairs(prs, kps, n_hyp=512, homography=True)
    base = gv.verify_pairs(plain, kps, n_hyp=512)
    assert len(got) == len(base) == 3
    for pr, b, kind in zip(got, base, tv.KINDS):
        c = case(kind)
        g = gv.two_view_geometry(c["kp1"], c["kp2"], c["matches"],
                                 pair=(pr.img_inx_1, pr.img_inx_2), n_hyp=512)
        assert pr.config == g["config"] and pr.h_count == g["h_count"]
        assert pr.h_ratio == g["h_ratio"]
        np.testing.assert_array_equal(pr.H, g["H"])
        np.testing.assert_array_equal(pr.F, g["F"])
        # the verified subset and .matches stay the F result, with and without the keyword
        assert pr.matches == b.matches == [tuple(c["matches"][i]) for i in g["f_inliers"]]
        np.testing.assert_array_equal(pr.F, b.F)
        assert not hasattr(b, "H") and not hasattr(b, "config") and not hasattr(b, "h_count")
