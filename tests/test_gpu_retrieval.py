"""GPU: sfm_vocab_assign / sfm_bow_hist / sfm_bow_neighbours, retrieval.select_pairs and
reconstruct(pairs=...) against the numpy restatement (retrieval_ref.py), byte for byte."""
import numpy as np
import pytest
import torch

import incremental
import reconstruction as R
import retrieval
import retrieval_cases as cases
import retrieval_ref as ref
import sfmcore

pytestmark = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_assign(ctx, desc, n_kp, vocab):
    rw, rd = ref.assign(desc, n_kp, vocab)
    word, dist = ctx.vocab_assign(T(desc), T(n_kp), T(vocab))
    word, dist = word.cpu().numpy(), dist.cpu().numpy()
    assert word.dtype == np.int32 and word.tobytes() == rw.tobytes()
    assert dist.dtype == np.int32 and dist.tobytes() == rd.tobytes()
    return rw


@pytest.mark.parametrize("k_max", [100, 512])
@pytest.mark.parametrize("n_words", [1, 31, 33, 129, 257, 1000])
def test_assign_shapes(ctx, n_words, k_max):
    desc, n_kp, vocab = cases.random_case(100 * n_words + k_max, 4, k_max, n_words)
    assert {0, 1, k_max} <= set(n_kp.tolist())
    _check_assign(ctx, desc, n_kp, vocab)


def test_assign_ties_resolve_to_the_lowest_index(ctx):
    for seed, n_words in ((1, 257), (2, 129), (3, 1000)):
        desc, n_kp, vocab = cases.tie_case(seed, n_words=n_words)
        word = _check_assign(ctx, desc, n_kp, vocab)
        # tied across 128-word groups: some winners have an equal word in a later group
        v = word[word >= 0]
        later = [(vocab[j + 1:] == vocab[j]).all(1).any() for j in np.unique(v)]
        assert np.mean(later) > 0.5


def test_assign_extremes(ctx):
    for desc, n_kp, vocab in cases.extreme_case():
        _check_assign(ctx, desc, n_kp, vocab)
    d = np.zeros((1, 1, 128), np.uint8)
    _, dist = ctx.vocab_assign(T(d), T(np.array([1], np.int32)), T(np.full((1, 128), 255, np.uint8)))
    assert int(dist[0, 0]) == 128 * 255 * 255


def test_assign_65536_words(ctx):
    desc, n_kp, vocab = cases.random_case(77, 4, 64, 65536)
    n_kp[:] = [64, 0, 1, 64]
    word = _check_assign(ctx, desc, n_kp, vocab)
    assert word.max() >= 1 << 15                  # indices beyond 16 signed bits are reached
    # the last word wins where it must
    desc[0, 0] = vocab[65535]
    vocab[:65535][(vocab[:65535] == vocab[65535]).all(1)] ^= 1
    assert _check_assign(ctx, desc, n_kp, vocab)[0, 0] == 65535


def test_assign_without_dist_and_with_out(ctx):
    desc, n_kp, vocab = cases.random_case(9, 3, 100, 129)
    rw, rd = ref.assign(desc, n_kp, vocab)
    word, dist = ctx.vocab_assign(T(desc), T(n_kp), T(vocab), with_dist=False)
    assert dist is None and word.cpu().numpy().tobytes() == rw.tobytes()
    out = (torch.full((3, 100), 7, dtype=torch.int32, device="cuda"),
           torch.full((3, 100), 7, dtype=torch.int32, device="cuda"))
    got = ctx.vocab_assign(T(desc), T(n_kp), T(vocab), out=out)
    assert got[0] is out[0] and out[0].cpu().numpy().tobytes() == rw.tobytes()
    assert out[1].cpu().numpy().tobytes() == rd.tobytes()
    with pytest.raises(sfmcore.SfmCoreError):
        ctx.vocab_assign(T(desc), T(n_kp), T(vocab[:, :64]))
    with pytest.raises(sfmcore.SfmCoreError, match="sfm_vocab_assign"):
        ctx.vocab_assign(T(desc), T(n_kp), T(vocab[:0]))


def test_assign_equals_the_matcher_nearest_neighbour(ctx):
    """An independent implementation: match_batch without cross check or ratio test, the
    vocabulary as a seventh image."""
    rng = np.random.Generator(np.random.PCG64(31))
    desc = rng.integers(0, 256, size=(7, 512, 128), dtype=np.uint8)
    near = rng.random((6, 512)) < 0.5
    pick = rng.integers(0, 512, size=(6, 512))
    d2 = np.clip(desc[6][pick].astype(int) + rng.integers(-3, 4, size=(6, 512, 128)), 0, 255)
    desc[:6] = np.where(near[..., None], d2.astype(np.uint8), desc[:6])
    n_kp = np.full(7, 512, np.int32)
    pairs = np.stack([np.arange(6), np.full(6, 6)], 1).astype(np.int32)
    cnt, mt, dist = ctx.match_batch(T(desc), T(n_kp), T(pairs), cross_check=sfmcore.XC_NONE)
    word, wd = ctx.vocab_assign(T(desc[:6]), T(n_kp[:6]), T(desc[6]))
    cnt, mt, dist = cnt.cpu().numpy(), mt.cpu().numpy(), dist.cpu().numpy()
    assert (cnt == 512).all()
    assert (mt[:, :, 0] == np.arange(512)[None, :]).all()
    assert mt[:, :, 1].astype(np.int32).tobytes() == word.cpu().numpy().tobytes()
    assert dist.tobytes() == wd.cpu().numpy().tobytes()


def _check_hist_neighbours(ctx, word, n_kp, n_words, weight=None):
    n_img = word.shape[0]
    rh = ref.hist(word, n_kp, n_words)
    hist = ctx.bow_hist(T(word), T(n_kp), n_words)
    assert hist.dtype == torch.uint16 and hist.cpu().numpy().tobytes() == rh.tobytes()
    wt = ref.idf_weights(rh) if weight is None else weight
    if weight is None:
        assert retrieval.idf_weights(hist).cpu().numpy().tobytes() == wt.tobytes()
    for k in sorted({1, 5, n_img - 1, n_img + 3} - {0}):
        rn, rs = ref.neighbours(rh, wt, k)
        nbr, sc = ctx.bow_neighbours(hist, T(wt), k)
        assert nbr.shape == (n_img, k) and nbr.cpu().numpy().tobytes() == rn.tobytes()
        assert sc.dtype == torch.int64 and sc.cpu().numpy().tobytes() == rs.tobytes()
    return rh, wt


@pytest.mark.parametrize("n_words", [1, 33, 4096])
@pytest.mark.parametrize("n_img", [1, 2, 3, 33, 72])
def test_hist_and_neighbours(ctx, n_img, n_words):
    word, n_kp = cases.hist_case(n_img * 10 + n_words, n_img, n_words)
    rh, wt = _check_hist_neighbours(ctx, word, n_kp, n_words)
    if n_img >= 33:
        rn, _ = ref.neighbours(rh, wt, n_img - 1)
        assert (rn[5] == -1).all() and not (rn == 5).any()      # the image without descriptors
        row = list(rn[1])
        if 0 in row:                                            # identical images 0, 2, 20
            assert row.index(0) < row.index(2) < row.index(20)
    # weights at the ends of their range
    rng = np.random.Generator(np.random.PCG64(n_img))
    w2 = rng.choice(np.array([0, 1, 65535], np.int32), size=n_words).astype(np.int32)
    _check_hist_neighbours(ctx, word, n_kp, n_words, weight=w2)


def test_hist_counts_up_to_k_max_and_skips_out_of_range(ctx):
    word = np.zeros((2, 8192), np.int32)
    word[1, ::2] = 3
    word[1, 1::4] = -1
    n_kp = np.array([8192, 8000], np.int32)
    h = ctx.bow_hist(T(word), T(n_kp), 5).cpu().numpy()
    assert h.tobytes() == ref.hist(word, n_kp, 5).tobytes() and h[0, 0] == 8192
    # the largest score: 65535 * 65535 per word needs the int64
    hist = np.full((2, 3), 65535, np.uint16)
    wt = np.full(3, 65535, np.int32)
    nbr, sc = ctx.bow_neighbours(T(hist), T(wt), 1)
    assert nbr.cpu().tolist() == [[1], [0]] and sc.cpu().tolist() == [[3 * 65535 * 65535]] * 2
    with pytest.raises(sfmcore.SfmCoreError):
        ctx.bow_neighbours(T(hist), T(np.array([0, 65536, 1], np.int32)), 1)
    with pytest.raises(sfmcore.SfmCoreError):
        ctx.bow_neighbours(T(hist), T(wt), 0)


def test_zero_weight_pairs_are_excluded(ctx):
    h = np.zeros((3, 4), np.uint16)
    h[0, 0], h[1, 0] = 3, 2
    h[1, 1], h[2, 1] = 1, 4
    wt = np.array([0, 5, 7, 7], np.int32)
    nbr, sc = ctx.bow_neighbours(T(h), T(wt), 2)
    assert nbr.cpu().tolist() == [[-1, -1], [2, -1], [1, -1]]
    assert sc.cpu().tolist() == [[0, 0], [5, 0], [5, 0]]
    rn, rs = ref.neighbours(h, wt, 2)
    assert nbr.cpu().numpy().tobytes() == rn.tobytes() and sc.cpu().numpy().tobytes() == rs.tobytes()


@pytest.mark.parametrize("lloyd", [0, 2])
def test_select_pairs_on_the_local_scene(lloyd):
    s = cases.local_scene()
    r = cases.local_scene_ref(lloyd)
    pairs, info = retrieval.select_pairs(s["desc"], s["n_kp"], return_info=True,
                                         **dict(cases.SCENE_PARAMS, lloyd=lloyd))
    assert info["vocab"].tobytes() == r["vocab"].tobytes()
    assert info["words"].tobytes() == r["words"].tobytes()
    assert info["hist"].tobytes() == r["hist"].tobytes()
    assert info["weight"].tobytes() == r["weight"].tobytes()
    assert info["neighbours"].tobytes() == r["neighbours"].tobytes()
    assert info["scores"].tobytes() == r["scores"].tobytes()
    assert pairs.dtype == np.int32 and pairs.tobytes() == r["pairs"].tobytes()
    assert {"vocabulary", "assign", "hist", "neighbours"} <= set(info["timings"])
    # the plain call returns the same list
    again = retrieval.select_pairs(s["desc"], s["n_kp"], **dict(cases.SCENE_PARAMS, lloyd=lloyd))
    assert again.tobytes() == pairs.tobytes()


def _median_reprojection(rec, scene):
    tptr, timg, tkp = rec.tracks
    obs_track = np.repeat(np.arange(len(tptr) - 1), np.diff(tptr))
    use = rec.has_point[obs_track] & rec.registered[timg]
    pts_ids, pt_idx = np.unique(obs_track[use], return_inverse=True)
    err = R.reprojection_errors(rec.cams, scene["pp"], rec.points[pts_ids], timg[use],
                                pt_idx.astype(np.int32), scene["kps"][timg[use], tkp[use]])
    return float(np.median(err))


# The retrieval run's median reprojection error may exceed the all-pairs run's by at most this
# many pixels: a tenth of the scene's keypoint noise sigma (0.5 px).  Both runs see the same noisy
# keypoints; the retrieval run only drops a few percent of the verified matches, which moves the
# median of ~10^5 residuals by its sampling error, of the order sigma / sqrt(10^4) = 0.005 px.
REPROJ_MARGIN_PX = 0.05


def test_reconstruct_with_retrieval_and_explicit_pairs():
    s = cases.local_scene()
    intr = np.c_[s["cams"][:, 6:8], s["pp"]]
    n = cases.SCENE_N_IMG
    full = incremental.reconstruct(s["desc"], s["kps"], s["n_kp"], intr)
    all_pairs = np.stack(np.triu_indices(n, 1), axis=1).astype(np.int32)
    assert full.pairs.tobytes() == all_pairs.tobytes() and "select_pairs" not in full.timings

    ret = incremental.reconstruct(s["desc"], s["kps"], s["n_kp"], intr, pairs="retrieval",
                                  retrieval=dict(k=24, n_words=4096, seed=7))
    assert ret.pairs.tobytes() == cases.local_scene_ref()["pairs"].tobytes()
    assert ret.timings["select_pairs"] > 0
    m_full, m_ret = _median_reprojection(full, s), _median_reprojection(ret, s)
    print(f"registered {int(full.registered.sum())} / {int(ret.registered.sum())} of {n}; "
          f"n_verified {full.n_verified} / {ret.n_verified} "
          f"({ret.n_verified / full.n_verified:.4f}); median reprojection {m_full:.4f} / "
          f"{m_ret:.4f} px; pairs {len(full.pairs)} / {len(ret.pairs)}")
    assert (ret.registered == full.registered).all()
    assert ret.n_verified >= 0.98 * full.n_verified
    assert m_ret <= m_full + REPROJ_MARGIN_PX

    # pairs="retrieval" with no retrieval dict: every default of select_pairs
    dflt = incremental.reconstruct(s["desc"], s["kps"], s["n_kp"], intr, pairs="retrieval")
    assert dflt.pairs.tobytes() == cases.default_ref(False)["pairs"].tobytes()
    m_dflt = _median_reprojection(dflt, s)
    print(f"defaults: pairs {len(dflt.pairs)}; registered {int(dflt.registered.sum())}; "
          f"n_verified {dflt.n_verified} ({dflt.n_verified / full.n_verified:.4f}); "
          f"median reprojection {m_dflt:.4f} px")
    assert 0 < 2 * len(dflt.pairs) <= len(all_pairs)
    assert (dflt.registered == full.registered).all()
    assert dflt.n_verified >= 0.98 * full.n_verified
    assert m_dflt <= m_full + REPROJ_MARGIN_PX

    # the explicit all-pairs list (shuffled, with a duplicate) is the default run, bit for bit
    rng = np.random.Generator(np.random.PCG64(1))
    given = np.concatenate([all_pairs[rng.permutation(len(all_pairs))], all_pairs[:3]])
    exp = incremental.reconstruct(s["desc"], s["kps"], s["n_kp"], intr, pairs=given)
    assert exp.pairs.tobytes() == all_pairs.tobytes()
    assert exp.cams.tobytes() == full.cams.tobytes()
    assert exp.points.tobytes() == full.points.tobytes()
    assert (exp.has_point == full.has_point).all() and (exp.registered == full.registered).all()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(exp.tracks, full.tracks))


def test_defaults_on_a_small_collection():
    """16 images, 16384 descriptors: the default n_words (65536) exceeds the collection; the
    vocabulary-size rule gives 2048 words, the list equals the reference's (which meets the recall
    condition, test_retrieval_cpu.py), and reconstruct(pairs="retrieval") with no retrieval dict
    builds the all-pairs run's model."""
    s = cases.small_scene()
    r = cases.default_ref(True)
    pairs, info = retrieval.select_pairs(s["desc"], s["n_kp"], return_info=True)
    assert info["vocab"].shape == (2048, 128) and info["vocab"].tobytes() == r["vocab"].tobytes()
    assert info["words"].tobytes() == r["words"].tobytes()
    assert info["neighbours"].tobytes() == r["neighbours"].tobytes()
    assert info["scores"].tobytes() == r["scores"].tobytes()
    assert len(pairs) > 0 and pairs.tobytes() == r["pairs"].tobytes()
    intr = np.c_[s["cams"][:, 6:8], s["pp"]]
    full = incremental.reconstruct(s["desc"], s["kps"], s["n_kp"], intr)
    ret = incremental.reconstruct(s["desc"], s["kps"], s["n_kp"], intr, pairs="retrieval")
    m_full, m_ret = _median_reprojection(full, s), _median_reprojection(ret, s)
    print(f"registered {int(full.registered.sum())} / {int(ret.registered.sum())} of 16; "
          f"n_verified {full.n_verified} / {ret.n_verified}; median reprojection {m_full:.4f} / "
          f"{m_ret:.4f} px; pairs {len(full.pairs)} / {len(ret.pairs)}")
    assert ret.pairs.tobytes() == r["pairs"].tobytes()
    assert full.registered.all() and ret.registered.all()
    assert ret.n_verified >= 0.98 * full.n_verified
    assert m_ret <= m_full + REPROJ_MARGIN_PX


def test_degenerate_inputs_and_argument_kinds(ctx):
    s = cases.small_scene()
    keys = {"vocab", "words", "hist", "weight", "neighbours", "scores", "timings"}
    full_keys = set(retrieval.select_pairs(s["desc"][:2], s["n_kp"][:2], return_info=True)[1])
    assert full_keys == keys
    for desc, n_kp in ((s["desc"][:1], s["n_kp"][:1]),                      # one image
                       (s["desc"][:3], np.zeros(3, np.int32)),              # no descriptor
                       (s["desc"][:0], s["n_kp"][:0])):                     # no image
        pairs, info = retrieval.select_pairs(desc, n_kp, k=4, return_info=True)
        assert pairs.shape == (0, 2) and pairs.dtype == np.int32 and set(info) == keys
        assert info["words"].shape == desc.shape[:2] and (info["words"] == -1).all()
        assert info["neighbours"].shape == (len(desc), 4) and (info["neighbours"] == -1).all()
        assert info["scores"].dtype == np.int64 and info["hist"].dtype == np.uint16
        assert retrieval.select_pairs(desc, n_kp).shape == (0, 2)
    with pytest.raises(TypeError, match="refine_vocabulary"):
        retrieval.refine_vocabulary(s["desc"][0, :8], s["desc"][:2], s["n_kp"][:2], 1)


@pytest.mark.parametrize("bad", [[[1, 1]], [[2, 1]], [[0, 72]], [[-1, 3]], [0, 1], [[0.0, 1.0]]])
def test_reconstruct_rejects_malformed_pairs(bad):
    s = cases.local_scene()
    intr = np.c_[s["cams"][:, 6:8], s["pp"]]
    with pytest.raises(ValueError):
        incremental.reconstruct(s["desc"], s["kps"], s["n_kp"], intr, pairs=np.array(bad))
    with pytest.raises(ValueError):
        incremental.reconstruct(s["desc"], s["kps"], s["n_kp"], intr, pairs="all")
