"""GPU: guided matching (sfm_guided_match_batch) against its CPU statement
tests/guided_ref.c — count, match[:count], dist[:count] and ncand byte for byte — and the opt-in
second pass of match_graph.GraphBuilder / incremental.reconstruct built on it.
"""
import functools

import numpy as np
import pytest

import geometric_verification as gv
import guided_cases as GC
import guided_ref
import incremental
import match_graph
import reconstruction as R
import sfmcore
import synth

pytestmark = pytest.mark.gpu

KEYS = ("desc", "n_kp", "kps", "pairs", "inl_count", "F", "norm")


def _dev(case):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(case[k])).cuda() for k in KEYS}


def _gpu(ctx, case, dev=None, **kw):
    d = dev or _dev(case)
    out = ctx.guided_match_batch(d["desc"], d["n_kp"], d["kps"], d["pairs"], d["inl_count"],
                                 d["F"], d["norm"], thr=case["thr"], with_ncand=True, **kw)
    return [t.cpu().numpy() for t in out]


def _ref(case, **kw):
    return guided_ref.batch(case["desc"], case["n_kp"], case["kps"], case["pairs"],
                            case["inl_count"], case["F"], case["norm"], thr=case["thr"], **kw)


def _assert_equal(got, want, pairs=None):
    """count, match[:count], dist[:count] and ncand byte for byte (entries from count on are
    unspecified)."""
    idx = range(len(want[0])) if pairs is None else pairs
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[3], want[3])
    for p in idx:
        n = int(want[0][p])
        np.testing.assert_array_equal(got[1][p, :n], want[1][p, :n])
        np.testing.assert_array_equal(got[2][p, :n], want[2][p, :n])


@functools.lru_cache(maxsize=None)
def _case(k_max):
    return GC.make_case(k_max)


# ---- 1. the case set ---------------------------------------------------------------------------

@pytest.mark.parametrize("rule", list(GC.RULES))
@pytest.mark.parametrize("k_max", [130, 520])
def test_case_set(ctx, k_max, rule):
    xc, ratio, md = GC.RULES[rule]
    case = _case(k_max)
    kw = dict(cross_check=xc, ratio=ratio, max_dist=md)
    want = _ref(case, **kw)
    assert int(want[0].sum()) > 50
    _assert_equal(_gpu(ctx, case, **kw), want)


# ---- 2. planted ties ----------------------------------------------------------------------------

def _tie_case(k_max=300):
    """Two images on one y under the horizontal F (everything is a candidate) except the train
    rows moved to y = 400, far outside the 2 px band."""
    rng = np.random.Generator(np.random.PCG64(5))
    desc = rng.integers(0, 256, size=(2, k_max, 128)).astype(np.uint8)
    kps = np.zeros((2, k_max, 2), np.float32)
    kps[..., 0] = rng.uniform(0, 600, size=(2, k_max))
    kps[..., 1] = 250.0
    norm = np.array([[300, 250, 0.01, 300, 250, 0.01]], np.float32)
    return dict(desc=desc, kps=kps, n_kp=np.array([k_max, k_max], np.int32),
                pairs=np.array([[0, 1]], np.int32), F=GC.HORIZONTAL_F[None].copy(), norm=norm,
                inl_count=np.array([100], np.int32), k_max=k_max, thr=4.0)


def _near(d, rng, n):
    """A descriptor n unit steps from d."""
    out = d.astype(np.int32).copy()
    dims = rng.choice(128, size=n, replace=False)
    out[dims] += np.where(out[dims] > 128, -1, 1)
    return out.astype(np.uint8)


def test_planted_ties(ctx):
    case = _tie_case()
    rng = np.random.Generator(np.random.PCG64(6))
    desc, kps = case["desc"], case["kps"]
    # query 0: equal train rows in one 128-group (10, 20); query 1: across groups (30, 200)
    desc[1, 10] = desc[1, 20] = desc[0, 0]
    desc[1, 30] = desc[1, 200] = desc[0, 1]
    # query 2: the lower twin (40) is outside the band, the higher (170) wins; the next candidate
    # (row 50, d^2 = 9) decides the ratio.  query 3: the same with a close next candidate (d^2 = 1)
    desc[1, 40] = desc[1, 170] = _near(desc[0, 2], rng, 4)      # d^2 = 4
    desc[1, 50] = _near(desc[0, 2], rng, 9)
    kps[1, 40, 1] = 400.0
    desc[1, 60] = desc[1, 260] = _near(desc[0, 3], rng, 4)
    desc[1, 70] = _near(desc[0, 3], rng, 5)
    kps[1, 60, 1] = 400.0
    # train row 90: equal queries 100 and 5 -> query 5 holds the mutual match
    desc[0, 100] = desc[0, 5] = desc[1, 90]
    # descriptor extremes: query 7 all 0 against train 95 all 255, the only candidate pairing
    desc[0, 7] = 0
    desc[1, 95] = 255
    kps[0, 7, 1] = kps[1, 95, 1] = 100.0
    none = _gpu(ctx, case, cross_check=0, ratio=None, max_dist=-1)
    _assert_equal(none, _ref(case, cross_check=0, ratio=None, max_dist=-1))
    m = {int(q): (int(t), int(d)) for (q, t), d in zip(none[1][0, :none[0][0]],
                                                       none[2][0, :none[0][0]])}
    assert m[0] == (10, 0) and m[1] == (30, 0)
    assert m[2] == (170, 4) and m[3] == (260, 4)
    assert m[7] == (95, 8323200) and none[3][0, 7] == 1
    ratio = _gpu(ctx, case, cross_check=0, ratio=(4, 5), max_dist=-1)
    _assert_equal(ratio, _ref(case, cross_check=0, ratio=(4, 5), max_dist=-1))
    kept = set(ratio[1][0, :ratio[0][0], 0].tolist())
    assert 0 not in kept and 1 not in kept      # the equal second candidate fails the ratio
    assert 2 in kept                            # 25 * 4 < 16 * 9: against row 50, not the twin
    assert 3 not in kept                        # 25 * 4 >= 16 * 5
    assert 7 in kept                            # a single candidate passes
    mutual = _gpu(ctx, case, cross_check=1, ratio=None, max_dist=-1)
    _assert_equal(mutual, _ref(case, cross_check=1, ratio=None, max_dist=-1))
    mm = dict(mutual[1][0, :mutual[0][0]].tolist())
    assert mm[5] == 90 and 100 not in mm


# ---- 3. all candidates: the new kernel against K1 ----------------------------------------------

@pytest.mark.parametrize("xc,ratio,max_dist", [(0, None, -1), (0, (4, 5), -1), (1, None, -1),
                                                (1, (4, 5), 30000)])
def test_all_candidates_equals_match_batch(ctx, xc, ratio, max_dist):
    case = GC.all_candidates_case(520, [520, 129, 33, 0, 513])
    d = _dev(case)
    got = _gpu(ctx, case, dev=d, cross_check=xc, ratio=ratio, max_dist=max_dist)
    count, match, dist = [t.cpu().numpy() for t in ctx.match_batch(
        d["desc"], d["n_kp"], d["pairs"], metric=sfmcore.METRIC_L2, cross_check=xc, ratio=ratio,
        max_dist=max_dist)]
    np.testing.assert_array_equal(got[0], count)
    assert int(count.sum()) > 100
    for p in range(len(count)):
        np.testing.assert_array_equal(got[1][p, :count[p]], match[p, :count[p]])
        np.testing.assert_array_equal(got[2][p, :count[p]], dist[p, :count[p]])


# ---- 4. against K2 ------------------------------------------------------------------------------

def test_ransac_inliers_are_candidates(ctx):
    import torch
    scene = synth.make_scene(4, 1024, 9)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    desc, kps, n_kp = T(scene["desc"]), T(scene["kps"]), T(scene["n_kp"])
    pairs = T(np.array([[0, 1], [1, 2], [3, 2]], np.int32))
    thr = 1.0
    count, match, dist = ctx.match_batch(desc, n_kp, pairs, ratio=(4, 5))
    rs = ctx.ransac_batch(kps, pairs, count, match, thr=thr)
    g = ctx.guided_match_batch(desc, n_kp, kps, pairs, rs["inl_count"], rs["F"], rs["norm"],
                               thr=thr, ratio=None, cross_check=sfmcore.XC_NONE, max_dist=-1,
                               with_ncand=True)
    gc, gm, gd, nc = [t.cpu().numpy() for t in g]
    count, match, dist, mask = [t.cpu().numpy() for t in (count, match, dist, rs["mask"])]
    for p in range(3):
        assert rs["inl_count"][p].item() >= 15
        best = np.full(1024, np.iinfo(np.int32).max, np.int64)
        best[gm[p, :gc[p], 0]] = gd[p, :gc[p]]
        inl = np.nonzero(mask[p, :count[p]])[0]
        qi = match[p, inl, 0]
        assert (nc[p, qi] >= 1).all()
        assert (best[qi] <= dist[p, inl]).all()


# ---- 5. skips -----------------------------------------------------------------------------------

def test_skips_leave_the_neighbours_alone(ctx):
    base = _case(130)
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    skipped = [2, 3, 4, 20, 24]
    case["inl_count"][2] = 14
    case["inl_count"][3] = -1
    case["norm"][4, 2] = 0.0
    case["norm"][20, 5] = 0.0
    case["F"][24, 4] = np.nan
    kw = dict(cross_check=1, ratio=(4, 5), max_dist=-1)
    want0 = _ref(base, **kw)
    got = _gpu(ctx, case, **kw)
    _assert_equal(got, _ref(case, **kw))
    for p in skipped:
        assert want0[0][p] > 0 and got[0][p] == 0 and not got[3][p].any()
    keep = [p for p in range(len(case["pairs"])) if p not in skipped]
    np.testing.assert_array_equal(got[0][keep], want0[0][keep])
    np.testing.assert_array_equal(got[3][keep], want0[3][keep])
    for p in keep:
        n = want0[0][p]
        np.testing.assert_array_equal(got[1][p, :n], want0[1][p, :n])
        np.testing.assert_array_equal(got[2][p, :n], want0[2][p, :n])


# ---- 6. batch invariance ------------------------------------------------------------------------

def test_batch_invariance(ctx):
    import torch
    case = _case(520)
    kw = dict(cross_check=1, ratio=(4, 5), max_dist=60000)
    d = _dev(case)
    full = _gpu(ctx, case, dev=d, **kw)
    P = len(case["pairs"])

    def sub(idx, with_ncand=True, out=None):
        ix = torch.from_numpy(np.asarray(idx)).cuda()
        o = ctx.guided_match_batch(d["desc"], d["n_kp"], d["kps"], d["pairs"][ix].contiguous(),
                                   d["inl_count"][ix].contiguous(), d["F"][ix].contiguous(),
                                   d["norm"][ix].contiguous(), thr=case["thr"],
                                   with_ncand=with_ncand, out=out, **kw)
        return o

    def same(o, idx, with_ncand=True):
        o = [t.cpu().numpy() for t in o]
        np.testing.assert_array_equal(o[0], full[0][idx])
        if with_ncand:
            np.testing.assert_array_equal(o[3], full[3][idx])
        for k, p in enumerate(idx):
            n = full[0][p]
            np.testing.assert_array_equal(o[1][k, :n], full[1][p, :n])
            np.testing.assert_array_equal(o[2][k, :n], full[2][p, :n])

    perm = np.random.Generator(np.random.PCG64(1)).permutation(P)
    same(sub(perm), perm)                                   # shuffled
    same(sub(np.arange(0, 7)), np.arange(0, 7))             # split
    same(sub(np.arange(7, P)), np.arange(7, P))
    same(sub(np.array([4])), np.array([4]))                 # alone
    same(sub(perm, with_ncand=False), perm, with_ncand=False)   # out_ncand NULL
    bufs = sub(perm)
    for t in bufs:
        t.fill_(-7)
    idx2 = perm[::-1].copy()
    assert sub(idx2, out=bufs)[1].data_ptr() == bufs[1].data_ptr()   # out= buffers reused
    same(bufs, idx2)


# ---- 7. end to end, pair level ------------------------------------------------------------------

@pytest.mark.parametrize("seed", [3, 4, 5])
def test_guided_builder_pair(ctx, seed):
    """make_scene(6, 1024, seed, desc_noise=24), pair (2, 3): the builder with guided matching on
    (thr 4 px^2, max_dist 160000) equals the four-call composition byte for byte, verifies at
    least twice the default builder's inliers, and at least 98 % of them join keypoints of one
    3-D point.

    The same pipeline on the CPU (oracle.match, oracle.ransac_f, guided_ref.batch,
    oracle.ransac_f; default inliers -> guided inliers, gain, true inliers):
        seed 3:  90 -> 233  2.59x  232 of 233 (99.57 %)
        seed 4:  67 -> 216  3.22x  215 of 216 (99.54 %)
        seed 5:  68 -> 221  3.25x  220 of 221 (99.55 %)
    so the two bars (2x, 98 %) are cleared with room by the reference itself."""
    import torch
    scene = synth.make_scene(6, 1024, seed, desc_noise=24)
    opts = dict(thr=4.0, max_dist=160000)
    gb0 = match_graph.GraphBuilder(scene["desc"], scene["kps"], scene["n_kp"])
    gb = match_graph.GraphBuilder(scene["desc"], scene["kps"], scene["n_kp"], guided=opts)
    pairs_t = torch.from_numpy(np.array([[2, 3], [0, 1]], np.int32)).cuda()
    c0, m0, d0, rs0 = gb0.run(pairs_t)
    plain = int(rs0["inl_count"][0].item())
    # the four calls
    c1, m1, _ = ctx.match_batch(gb.desc, gb.n_kp, pairs_t, **gb0.match_kw)
    r1 = ctx.ransac_batch(gb.kps, pairs_t, c1, m1, **gb0.ransac_kw)
    c2, m2, d2 = ctx.guided_match_batch(gb.desc, gb.n_kp, gb.kps, pairs_t, r1["inl_count"],
                                        r1["F"], r1["norm"], thr=4.0, ratio=(4, 5),
                                        cross_check=sfmcore.XC_MUTUAL, max_dist=160000,
                                        min_inliers=15)
    r2 = ctx.ransac_batch(gb.kps, pairs_t, c2, m2, **gb0.ransac_kw)
    count, match, dist, rs = gb.run(pairs_t)
    assert torch.equal(count, c2)
    for p in range(2):
        n = int(c2[p].item())
        assert torch.equal(match[p, :n], m2[p, :n]) and torch.equal(dist[p, :n], d2[p, :n])
        assert torch.equal(rs["mask"][p, :n], r2["mask"][p, :n])
    for k in ("inl_count", "best_h", "F", "norm"):
        assert torch.equal(rs[k], r2[k])
    guided = int(rs["inl_count"][0].item())
    n = int(count[0].item())
    inl = rs["mask"][0, :n].cpu().numpy().astype(bool)
    mt = match[0, :n].cpu().numpy()[inl]
    pid = scene["point_ids"]
    true = (pid[2][mt[:, 0]] == pid[3][mt[:, 1]]) & (pid[2][mt[:, 0]] >= 0)
    print(f"seed {seed}: {plain} -> {guided} ({guided / plain:.2f}x), true {true.sum()} of "
          f"{len(true)} ({100 * true.mean():.2f} %)")
    assert guided == len(true)
    assert guided >= 2 * plain
    assert true.mean() >= 0.98


# ---- 8. end to end, driver level ----------------------------------------------------------------

def _median_error(rec, scene):
    tptr, timg, tkp = rec.tracks
    obs_track = np.repeat(np.arange(len(tptr) - 1), np.diff(tptr))
    use = rec.has_point[obs_track]
    pts_ids, pt_idx = np.unique(obs_track[use], return_inverse=True)
    err = R.reprojection_errors(rec.cams, scene["pp"], rec.points[pts_ids], timg[use],
                                pt_idx.astype(np.int32), scene["kps"][timg[use], tkp[use]])
    return float(np.median(err))


def test_reconstruct_guided():
    scene = synth.make_scene(10, 1024, seed=21, k1_range=0.02, desc_noise=24)
    intr = np.c_[scene["cams"][:, 6:8], scene["pp"]]
    rec0 = incremental.reconstruct(scene["desc"], scene["kps"], scene["n_kp"], intr)
    rec = incremental.reconstruct(scene["desc"], scene["kps"], scene["n_kp"], intr, guided=True)
    print(f"registered {rec0.registered.sum()} -> {rec.registered.sum()}, n_verified "
          f"{rec0.n_verified} -> {rec.n_verified}, median error {_median_error(rec, scene):.3f}")
    assert rec.registered.sum() >= rec0.registered.sum()
    assert rec.n_verified > rec0.n_verified
    assert _median_error(rec, scene) < 0.8


def test_guided_match_pair_equals_the_batch():
    import torch
    scene = synth.make_scene(6, 1024, 3, desc_noise=24)
    a, b = 2, 3
    gb = match_graph.GraphBuilder(scene["desc"], scene["kps"], scene["n_kp"], guided=True)
    pairs_t = torch.from_numpy(np.array([[0, 5], [a, b]], np.int32)).cuda()
    count, match, dist, rs = gb.run(pairs_t)
    n = int(count[1].item())
    one = gv.guided_match_pair(scene["kps"][a], scene["kps"][b], scene["desc"][a],
                               scene["desc"][b], pair=(a, b), guided=True)
    np.testing.assert_array_equal(one["matches"], match[1, :n].cpu().numpy())
    np.testing.assert_array_equal(one["dist"], dist[1, :n].cpu().numpy())
    np.testing.assert_array_equal(one["inliers"],
                                  np.nonzero(rs["mask"][1, :n].cpu().numpy())[0])
    assert one["count"] == int(rs["inl_count"][1].item()) and one["verified"]
    np.testing.assert_array_equal(
        one["F"], gv.denormalize_F(rs["F"][1].cpu().numpy(), rs["norm"][1].cpu().numpy()))
    assert one["first_count"] < one["count"]
