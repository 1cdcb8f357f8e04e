"""GPU parity: the two-view pose batch (sfm_two_view_pose_batch) against its CPU statement
tests/pose_ref.c, EVERY BYTE of E, R, t, stat and median_key: random noisy pairs (junk essential
matrices, ties of the cheirality vote, distortion, a k_max that is no multiple of 16), the
lane-stride boundaries of the fixed-order sums, a mixed batch that is permuted, split and
interleaved with the F and H batches, a swapped pair, the public layer of geometric_verification,
and reconstruct(init_pair="pose")."""
import numpy as np
import pytest

import geometric_verification as gv
import incremental
import pose_ref
import reconstruction as R
import synth
import two_view_cases as tv

pytestmark = pytest.mark.gpu

INTR = np.array([tv.F_PX, 0.0, tv.PP[0], tv.PP[1]])
KEYS = ("E", "R", "t", "stat", "median_key")
_CASES = {}


def case(kind, seed=0):
    if (kind, seed) not in _CASES:
        _CASES[(kind, seed)] = tv.make(kind, seed=seed)
    return _CASES[(kind, seed)]


def dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def run_pose(ctx, kps, intr, pairs, count, match, mask, inl, **kw):
    import torch
    out = ctx.two_view_pose_batch(*dev(kps, intr, pairs, count, match, mask, inl), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_same_bytes(got, want, rows=None, what=""):
    for k in KEYS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if rows is not None:
            g = g[rows]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        np.testing.assert_array_equal(g.view(np.uint8), w.view(np.uint8), err_msg=f"{what} {k}")


def random_batch(seed, P=200, n_img=12, k_max=77):
    """Random keypoints, random matches and masks with 8..40 inliers per pair, k1 != 0 on every
    second image, images in either order."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kps = (rng.uniform(0.0, 1.0, size=(n_img, k_max, 2)) * [tv.W, tv.H]).astype(np.float32)
    intr = np.tile(INTR, (n_img, 1))
    intr[:, 0] = rng.uniform(800.0, 1200.0, size=n_img)
    intr[1::2, 1] = rng.uniform(-0.05, 0.05, size=len(intr[1::2]))
    pairs = np.zeros((P, 2), np.int32)
    count = np.zeros(P, np.int32)
    match = np.zeros((P, k_max, 2), np.int32)
    mask = np.zeros((P, k_max), np.uint8)
    for p in range(P):
        pairs[p] = rng.choice(n_img, size=2, replace=False)
        n_inl = 8 + p % 33
        M = int(rng.integers(n_inl, k_max + 1))
        count[p] = M
        match[p, :M, 0] = rng.permutation(k_max)[:M]
        match[p, :M, 1] = rng.permutation(k_max)[:M]
        mask[p, rng.permutation(M)[:n_inl]] = 1
    return kps, intr, pairs, count, match, mask, mask.sum(1).astype(np.int32)


def test_random_noisy_pairs_bit_exact(ctx):
    args = random_batch(5)
    got = run_pose(ctx, *args, min_inliers=8)
    want = pose_ref.pose_batch(*args, min_inliers=8)
    assert_same_bytes(got, want, what="random")
    st = want["stat"]
    assert (st[:, 0] == 0).all() and (st[:, 7] == args[6]).all()
    nf = st[:, 2:6]
    best = st[:, 1]
    # junk essential matrices: the vote ties on some pairs and the lowest index wins there
    tied = (np.sort(nf, axis=1)[:, -1] == np.sort(nf, axis=1)[:, -2])
    assert tied.any()
    assert (best == np.argmax(nf, axis=1)).all()
    assert len(set(best.tolist())) == 4


BOUNDARY_INLIERS = [7, 8, 9, 63, 64, 65, 128, 129]


def boundary_batch():
    """The general case's true inliers, `n` of them per pair spread over the 400 matches with
    masked-out entries (planted outliers and the unused inliers) in between."""
    c = case("general")
    rng = np.random.Generator(np.random.PCG64(11))
    P, k_max = len(BOUNDARY_INLIERS), 400
    kps = np.stack([c["kp1"], c["kp2"]])
    match = np.tile(c["matches"][None], (P, 1, 1)).astype(np.int32)
    mask = np.zeros((P, k_max), np.uint8)
    for p, n in enumerate(BOUNDARY_INLIERS):
        mask[p, np.sort(rng.choice(np.arange(c["n_out"], k_max), size=n, replace=False))] = 1
    pairs = np.tile(np.array([[0, 1]], np.int32), (P, 1))
    count = np.full(P, k_max, np.int32)
    return kps, np.tile(INTR, (2, 1)), pairs, count, match, mask, mask.sum(1).astype(np.int32)


def test_lane_stride_boundaries(ctx):
    args = boundary_batch()
    got = run_pose(ctx, *args, min_inliers=8)
    want = pose_ref.pose_batch(*args, min_inliers=8)
    assert_same_bytes(got, want, what="boundaries")
    assert want["stat"][:, 0].tolist() == [1] + [0] * 7
    assert want["stat"][1:, 7].tolist() == BOUNDARY_INLIERS[1:]
    for k in ("E", "R", "t", "median_key"):
        assert not got[k][0].any()
    assert not got["stat"][0, 1:].any()


def mixed_batch(ctx):
    """The three two-view kinds verified by the F batch on the GPU, a pair below 8 matches
    (inl_count -1) and pairs between 8 inliers and min_inliers.  Returns the pose batch's inputs
    as numpy arrays (mask / inl_count are the F batch's outputs)."""
    import torch
    ids = {"general": (2, 5), "plane": (0, 3), "rot": (4, 1)}
    k_max = 403
    kps = np.zeros((7, k_max, 2), np.float32)
    items = []
    for kind, (a, b) in ids.items():
        c = case(kind)
        kps[a, :400], kps[b, :400] = c["kp1"], c["kp2"]
        items.append((a, b, 400))
    g = case("general", 1)
    kps[6, :400] = g["kp2"]
    items += [(2, 6, 5), (5, 2, 400), (0, 4, 12), (3, 0, 40)]
    pairs = np.array([[a, b] for a, b, _ in items], np.int32)
    count = np.array([M for *_, M in items], np.int32)
    match = np.zeros((len(items), k_max, 2), np.int32)
    match[:, :, 0] = match[:, :, 1] = np.arange(k_max)
    kd, pd, cd, md = dev(kps, pairs, count, match)
    rs = ctx.ransac_batch(kd, pd, cd, md, n_hyp=512)
    torch.cuda.synchronize()
    intr = np.tile(INTR, (7, 1))
    intr[3, 1], intr[5, 1] = 0.01, -0.02
    return (kps, intr, pairs, count, match, rs["mask"].cpu().numpy(),
            rs["inl_count"].cpu().numpy())


def test_mixed_batch_invariances(ctx):
    import torch
    args = mixed_batch(ctx)
    kps, intr, pairs, count, match, mask, inl = args
    assert inl[3] == -1 and (inl[:3] >= 15).all()
    want = pose_ref.pose_batch(*args)
    got = run_pose(ctx, *args)
    assert_same_bytes(got, want, what="mixed")
    assert want["stat"][:3, 0].tolist() == [0, 0, 0] and want["stat"][3, 0] == 1
    assert (want["stat"][inl < 15, 0] == 1).all()
    P = len(pairs)
    sub = lambda rows: (kps, intr, pairs[rows], count[rows], match[rows], mask[rows], inl[rows])
    # permuted
    perm = np.random.Generator(np.random.PCG64(3)).permutation(P)
    assert_same_bytes(run_pose(ctx, *sub(perm)), {k: want[k][perm] for k in KEYS}, what="perm")
    # split in two
    for rows in (np.arange(0, 3), np.arange(3, P)):
        assert_same_bytes(run_pose(ctx, *sub(rows)), {k: want[k][rows] for k in KEYS},
                          what="split")
    # interleaved with F and H batches on the same context (they share its workspace)
    d = dev(*args)
    kd, pd, cd, md = d[0], d[2], d[3], d[4]
    o1 = ctx.two_view_pose_batch(*d)
    ctx.ransac_batch(kd, pd, cd, md, n_hyp=256)
    o2 = ctx.two_view_pose_batch(*d)
    ctx.ransac_h_batch(kd, pd, cd, md, n_hyp=256)
    o3 = ctx.two_view_pose_batch(*d)
    torch.cuda.synchronize()
    for o in (o1, o2, o3):
        assert_same_bytes({k: v.cpu().numpy() for k, v in o.items()}, want, what="interleaved")
    # P = 0
    e = ctx.two_view_pose_batch(*dev(kps, intr, pairs[:0], count[:0], match[:0], mask[:0], inl[:0]))
    assert e["stat"].shape == (0, 8) and e["R"].shape == (0, 9)


def test_swapped_pair(ctx):
    c = case("general")
    kps = np.stack([c["kp1"], c["kp2"]])
    intr = np.tile(INTR, (2, 1))
    intr[1, 1] = 0.015
    mask = np.zeros((2, 400), np.uint8)
    mask[:, c["n_out"]:] = 1
    mask[:, 150::7] = 0
    match = np.tile(c["matches"][None], (2, 1, 1)).astype(np.int32)
    args = (kps, intr, np.array([[0, 1], [1, 0]], np.int32), np.full(2, 400, np.int32), match,
            mask, mask.sum(1).astype(np.int32))
    got = run_pose(ctx, *args)
    assert_same_bytes(got, pose_ref.pose_batch(*args), what="swapped")
    assert got["stat"][:, 0].tolist() == [0, 0]


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


def test_two_view_pose_and_verify_pairs(ctx):
    intr6 = np.tile(INTR, (6, 1))
    prs, kps = _pair_list()
    plain, _ = _pair_list()
    both, _ = _pair_list()
    got = gv.verify_pairs(prs, kps, n_hyp=512, poses=True, intrinsics=intr6)
    base = gv.verify_pairs(plain, kps, n_hyp=512)
    comp = gv.verify_pairs(both, kps, n_hyp=512, poses=True, intrinsics=intr6, homography=True)
    assert len(got) == len(base) == len(comp) == 3
    for pr, b, cp, kind in zip(got, base, comp, tv.KINDS):
        c = case(kind)
        a_, b_ = pr.img_inx_1, pr.img_inx_2
        tp = gv.two_view_pose(c["kp1"], c["kp2"], c["matches"], intr6[a_], intr6[b_],
                              pair=(a_, b_), n_hyp=512)
        # the batch on the same pair, from the F batch's mask
        kk = np.stack([c["kp1"], c["kp2"]])
        m = np.zeros((1, 400), np.uint8)
        m[0, tp["inliers"]] = 1
        o = run_pose(ctx, kk, intr6[[a_, b_]], np.array([[0, 1]], np.int32),
                     np.array([400], np.int32), c["matches"][None].astype(np.int32), m,
                     np.array([tp["count"]], np.int32))
        assert tp["status"] == 0 and o["stat"][0, 0] == 0
        np.testing.assert_array_equal(tp["R"].ravel(), o["R"][0])
        np.testing.assert_array_equal(tp["t"], o["t"][0])
        np.testing.assert_array_equal(tp["E"].ravel(), o["E"][0])
        assert tp["n_front_all"] == o["stat"][0, 2:6].tolist() and tp["best"] == o["stat"][0, 1]
        assert tp["n_front"] == o["stat"][0, 2 + o["stat"][0, 1]]
        assert tp["n_wide"] == o["stat"][0, 6]
        assert tp["tri_angle_deg"] == gv.key_to_degrees(float(o["median_key"][0]))
        for q in (pr, cp):
            np.testing.assert_array_equal(q.R, tp["R"])
            np.testing.assert_array_equal(q.t, tp["t"])
            assert (q.n_front, q.n_wide, q.tri_angle_deg, q.pose_status) == \
                (tp["n_front"], tp["n_wide"], tp["tri_angle_deg"], 0)
            np.testing.assert_array_equal(q.F, tp["F"])
            assert q.matches == b.matches
        assert cp.config in ("general", "planar_or_panoramic") and cp.H.shape == (3, 3)
        for name in ("R", "t", "n_front", "tri_angle_deg", "n_wide", "pose_status"):
            assert not hasattr(b, name)
    # what the poses say about the three kinds
    assert 9.0 < got[0].tri_angle_deg < 13.0 and got[0].n_wide > 0.9 * got[0].n_front
    assert got[2].tri_angle_deg < 0.5


def _reprojection_median(rec, scene):
    tptr, timg, tkp = rec.tracks
    obs_track = np.repeat(np.arange(len(tptr) - 1), np.diff(tptr))
    use = rec.has_point[obs_track] & rec.registered[timg]
    pts_ids, pt_idx = np.unique(obs_track[use], return_inverse=True)
    err = R.reprojection_errors(rec.cams, scene["pp"], rec.points[pts_ids], timg[use],
                                pt_idx.astype(np.int32), scene["kps"][timg[use], tkp[use]])
    return np.median(err), int(use.sum())


def test_reconstruct_init_pair_pose():
    """The scene of test_gpu_incremental.py's first test: every image registered, the same
    reprojection bound, and the seed pair has the most wide rays among the pairs tried."""
    scene = synth.make_scene(10, 1024, seed=21, k1_range=0.02)
    intr = np.c_[scene["cams"][:, 6:8], scene["pp"]]
    rec = incremental.reconstruct(scene["desc"], scene["kps"], scene["n_kp"], intr,
                                  init_pair="pose")
    assert rec.registered.all()
    med, n_use = _reprojection_median(rec, scene)
    assert n_use > 2000 and med < 0.8
    by_pair = {c["pair"]: c for c in rec.init_candidates}
    assert len(rec.init_candidates) == 45 and rec.gauge in rec.init_tried
    assert by_pair[rec.gauge]["status"] == 0
    assert by_pair[rec.gauge]["n_wide"] == max(by_pair[p]["n_wide"] for p in rec.init_tried)
    inl = [c["inliers"] for c in rec.init_candidates]
    assert inl == sorted(inl, reverse=True)


def test_reconstruct_pose_prefers_the_wide_pair():
    """Images 0 and 1 are near-duplicate views (image 1 = image 0's keypoints moved by 0.2 px
    noise, same descriptors): the pair with the most matches and no baseline.  "pose" seeds the
    model from a pair with a baseline instead."""
    scene = synth.make_scene(4, 768, seed=4, arc_deg=40.0)
    rng = np.random.Generator(np.random.PCG64(99))
    scene["kps"][1] = scene["kps"][0] + rng.normal(0.0, 0.2, size=scene["kps"][0].shape)
    scene["desc"][1] = scene["desc"][0]
    scene["cams"][1] = scene["cams"][0]
    intr = np.c_[scene["cams"][:, 6:8], scene["pp"]]
    rec = incremental.reconstruct(scene["desc"], scene["kps"], scene["n_kp"], intr,
                                  init_pair="pose")
    cands = rec.init_candidates
    assert cands[0]["pair"] == (0, 1) and cands[0]["inliers"] > 1.5 * cands[1]["inliers"]
    assert cands[0]["n_wide"] == 0
    assert rec.gauge is not None and rec.gauge != (0, 1)
    by_pair = {c["pair"]: c for c in cands}
    assert by_pair[rec.gauge]["n_wide"] == max(c["n_wide"] for c in cands) > 100
