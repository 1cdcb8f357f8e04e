"""GPU: sfm_vocab_assign_hamming / sfm_vocab_majority, retrieval.select_pairs and
reconstruct(pairs="retrieval") on binary (32-byte) descriptors against the numpy restatement
(retrieval_hamming_ref.py), byte for byte."""
import numpy as np
import pytest
import torch

import incremental
import reconstruction as R
import retrieval
import retrieval_hamming_cases as cases
import retrieval_hamming_ref as ref
import sfmcore

pytestmark = pytest.mark.gpu

# test_gpu_retrieval.REPROJ_MARGIN_PX and its reasoning: a tenth of the scene's keypoint noise
# sigma (0.5 px).  Both runs see the same noisy keypoints; dropping a few percent of the verified
# matches moves the median of ~10^5 residuals by its sampling error, ~ sigma / sqrt(10^4).
REPROJ_MARGIN_PX = 0.05


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _median_reprojection(rec, scene):
    tptr, timg, tkp = rec.tracks
    obs_track = np.repeat(np.arange(len(tptr) - 1), np.diff(tptr))
    use = rec.has_point[obs_track] & rec.registered[timg]
    pts_ids, pt_idx = np.unique(obs_track[use], return_inverse=True)
    err = R.reprojection_errors(rec.cams, scene["pp"], rec.points[pts_ids], timg[use],
                                pt_idx.astype(np.int32), scene["kps"][timg[use], tkp[use]])
    return float(np.median(err))


def _check_assign(ctx, desc, n_kp, vocab):
    rw, rd = ref.assign(desc, n_kp, vocab)
    word, dist = ctx.vocab_assign(T(desc), T(n_kp), T(vocab))
    word, dist = word.cpu().numpy(), dist.cpu().numpy()
    assert word.dtype == np.int32 and word.tobytes() == rw.tobytes()
    assert dist.dtype == np.int32 and dist.tobytes() == rd.tobytes()
    return rw, rd


# flattened rows 400, 650, 2048 against 256-row workgroups: across, across with a ragged tail, on
@pytest.mark.parametrize("n_img,k_max", [(4, 100), (5, 130), (4, 512)])
@pytest.mark.parametrize("n_words", [1, 31, 33, 127, 129, 257, 1000])
def test_assign_shapes(ctx, n_words, n_img, k_max):
    desc, n_kp, vocab = cases.random_case(100 * n_words + k_max, n_img, k_max, n_words)
    assert {0, 1, k_max} <= set(n_kp.tolist())
    _, rd = _check_assign(ctx, desc, n_kp, vocab)
    if n_words > 4:
        assert (rd[np.arange(k_max)[None, :] < n_kp[:, None]] <= 3).mean() > 0.2


def test_assign_fewer_rows_than_a_workgroup(ctx):
    desc, n_kp, vocab = cases.random_case(5, 4, 33, 129)      # 132 rows
    _check_assign(ctx, desc, n_kp, vocab)


def test_assign_ties_resolve_to_the_lowest_index(ctx):
    for seed, n_words in ((1, 257), (2, 129), (3, 1000)):
        desc, n_kp, vocab = cases.tie_case(seed, n_words=n_words)
        word, dist = _check_assign(ctx, desc, n_kp, vocab)
        v = word[word >= 0]
        assert set(dist[word >= 0].tolist()) == {0, 1}        # half of them one bit off a word
        # most winners have an identical word at a higher index, often in a later 128-word group
        later = [(vocab[j + 1:] == vocab[j]).all(1).any() for j in np.unique(v)]
        assert np.mean(later) > 0.5
        if n_words >= 257:     # 129 words leave a single word to the second group
            later_group = [(vocab[(j // 128 + 1) * 128:] == vocab[j]).all(1).any()
                           for j in np.unique(v)]
            assert np.mean(later_group) > 0.5


def test_assign_extremes(ctx):
    seen = 0
    for desc, n_kp, vocab in cases.extreme_case():
        _, rd = _check_assign(ctx, desc, n_kp, vocab)
        seen = max(seen, int(rd.max()))
    assert seen == 256
    one = np.array([1], np.int32)
    for a, b, want in ((0, 255, 256), (255, 0, 256), (255, 255, 0), (0, 0, 0)):
        word, dist = ctx.vocab_assign(T(np.full((1, 1, 32), a, np.uint8)), T(one),
                                      T(np.full((1, 32), b, np.uint8)))
        assert int(word[0, 0]) == 0 and int(dist[0, 0]) == want


def test_assign_65536_words(ctx):
    desc, n_kp, vocab = cases.random_case(77, 4, 64, 65536)
    n_kp[:] = [64, 0, 1, 64]
    word, _ = _check_assign(ctx, desc, n_kp, vocab)
    assert word.max() >= 1 << 15                  # indices beyond 16 signed bits are reached
    # the last word wins where it alone is nearest
    desc[0, 0] = vocab[65535]
    vocab[:65535][(vocab[:65535] == vocab[65535]).all(1)] ^= 1
    assert _check_assign(ctx, desc, n_kp, vocab)[0][0, 0] == 65535


def test_assign_without_dist_with_out_and_rejections(ctx):
    desc, n_kp, vocab = cases.random_case(9, 4, 100, 129)
    rw, rd = ref.assign(desc, n_kp, vocab)
    word, dist = ctx.vocab_assign(T(desc), T(n_kp), T(vocab), with_dist=False)
    assert dist is None and word.cpu().numpy().tobytes() == rw.tobytes()
    out = (torch.full((4, 100), 7, dtype=torch.int32, device="cuda"),
           torch.full((4, 100), 7, dtype=torch.int32, device="cuda"))
    got = ctx.vocab_assign(T(desc), T(n_kp), T(vocab), out=out)
    assert got[0] is out[0] and out[0].cpu().numpy().tobytes() == rw.tobytes()
    assert out[1].cpu().numpy().tobytes() == rd.tobytes()
    wide = np.zeros((4, 100, 128), np.uint8)
    with pytest.raises(sfmcore.SfmCoreError):
        ctx.vocab_assign(T(desc), T(n_kp), T(np.zeros((129, 128), np.uint8)))
    with pytest.raises(sfmcore.SfmCoreError):
        ctx.vocab_assign(T(wide), T(n_kp), T(vocab))
    with pytest.raises(sfmcore.SfmCoreError, match="sfm_vocab_assign_hamming"):
        ctx.vocab_assign(T(desc), T(n_kp), T(vocab[:0]))
    with pytest.raises(sfmcore.SfmCoreError):
        ctx.vocab_assign(T(np.zeros((4, 100, 64), np.uint8)), T(n_kp), T(np.zeros((9, 64), np.uint8)))


def test_assign_equals_the_matcher_nearest_neighbour(ctx):
    """An independent implementation: match_batch under METRIC_HAMMING without cross check, ratio
    test or distance cut, the vocabulary as a seventh image of 512 descriptors.  Distances are
    equal everywhere, and so are the indices: the matcher's Hamming kernel documents a
    lowest-index argmin too (csrc/match_hamming.hip).  The share of unique minima is printed."""
    desc, n_kp, vocab = cases.random_case(31, 6, 512, 512)
    n_kp = np.full(7, 512, np.int32)
    both = np.concatenate([desc, vocab[None]])
    pairs = np.stack([np.arange(6), np.full(6, 6)], 1).astype(np.int32)
    cnt, mt, dist = ctx.match_batch(T(both), T(n_kp), T(pairs), metric=sfmcore.METRIC_HAMMING,
                                    cross_check=sfmcore.XC_NONE)
    word, wd = ctx.vocab_assign(T(desc), T(n_kp[:6]), T(vocab))
    cnt, mt, dist = cnt.cpu().numpy(), mt.cpu().numpy(), dist.cpu().numpy()
    word, wd = word.cpu().numpy(), wd.cpu().numpy()
    assert (cnt == 512).all()
    assert (mt[:, :, 0] == np.arange(512)[None, :]).all()
    assert dist.tobytes() == wd.tobytes()
    d64, v64 = desc.view(np.uint64), vocab.view(np.uint64)
    pop = ref.popcount(d64[:, :, None, :] ^ v64[None, None]).sum(-1, dtype=np.int32)
    unique = (pop == pop.min(-1, keepdims=True)).sum(-1) == 1
    same = mt[:, :, 1] == word
    print(f"unique minima {unique.mean():.3f}; indices equal on tied rows "
          f"{same[~unique].mean() if (~unique).any() else 1.0:.3f}")
    assert 0.2 < unique.mean() < 1.0 and same[unique].all()
    assert same.all()


@pytest.mark.parametrize("n_words", [1, 129, 1000])
def test_majority_round(ctx, n_words):
    desc, n_kp, word, vocab = cases.majority_case(40 + n_words, n_words, n_img=5, k_max=130)
    valid = (np.arange(130)[None, :] < n_kp[:, None]) & (word >= 0) & (word < n_words)
    cnt = np.bincount(word[valid], minlength=n_words)
    if n_words > 5:
        assert cnt[:5].tolist() == [0, 1, 2, 3, 4]
    want = ref.majority_round(vocab, desc, n_kp, word)
    got = ctx.vocab_majority(T(desc), T(n_kp), T(word), T(vocab)).cpu().numpy()
    assert got.dtype == np.uint8 and got.tobytes() == want.tobytes()
    assert (got[cnt == 0] == vocab[cnt == 0]).all()           # no member: the input bytes
    assert (got != vocab).any() or n_words == 1
    # the words of a real assignment, and a caller-supplied out
    w2, _ = ref.assign(desc, n_kp, vocab)
    out = torch.zeros((n_words, 32), dtype=torch.uint8, device="cuda")
    assert ctx.vocab_majority(T(desc), T(n_kp), T(w2), T(vocab), out=out) is out
    assert out.cpu().numpy().tobytes() == ref.majority_round(vocab, desc, n_kp, w2).tobytes()


def test_majority_round_65536_words(ctx):
    desc, n_kp, word, vocab = cases.majority_case(3, 65536, n_img=4, k_max=64)
    word[2, :8] = 65535                                       # the last word has members
    n_kp[2] = max(int(n_kp[2]), 8)
    want = ref.majority_round(vocab, desc, n_kp, word)
    got = ctx.vocab_majority(T(desc), T(n_kp), T(word), T(vocab)).cpu().numpy()
    assert got.tobytes() == want.tobytes()
    assert (got[65535] != vocab[65535]).any() and (got[0] == vocab[0]).all()


def _check_info(info, pairs, r):
    for key in ("vocab", "words", "hist", "weight", "neighbours", "scores"):
        assert info[key].dtype == r[key].dtype and info[key].tobytes() == r[key].tobytes(), key
    assert pairs.dtype == np.int32 and pairs.tobytes() == r["pairs"].tobytes()


@pytest.mark.parametrize("lloyd", [0, 2])
def test_select_pairs_on_the_local_scene(lloyd):
    s = cases.local_scene()
    kw = dict(cases.SCENE_PARAMS, lloyd=lloyd)
    pairs, info = retrieval.select_pairs(s["desc"], s["n_kp"], return_info=True, **kw)
    _check_info(info, pairs, cases.local_scene_ref(lloyd))
    assert info["vocab"].shape == (4096, 32)
    assert {"vocabulary", "assign", "hist", "neighbours"} <= set(info["timings"])
    assert retrieval.select_pairs(s["desc"], s["n_kp"], **kw).tobytes() == pairs.tobytes()


def test_select_pairs_defaults_on_a_small_collection():
    s = cases.small_scene()
    pairs, info = retrieval.select_pairs(s["desc"], s["n_kp"], return_info=True)
    _check_info(info, pairs, cases.default_ref(True))
    assert info["vocab"].shape == (2048, 32) and len(pairs) > 0
    assert retrieval.select_pairs(s["desc"], s["n_kp"]).tobytes() == pairs.tobytes()


def test_degenerate_inputs_and_rejection():
    s = cases.small_scene()
    keys = {"vocab", "words", "hist", "weight", "neighbours", "scores", "timings"}
    assert set(retrieval.select_pairs(s["desc"][:2], s["n_kp"][:2], return_info=True)[1]) == keys
    for desc, n_kp in ((s["desc"][:1], s["n_kp"][:1]),                      # one image
                       (s["desc"][:3], np.zeros(3, np.int32)),              # no descriptor
                       (s["desc"][:0], s["n_kp"][:0])):                     # no image
        pairs, info = retrieval.select_pairs(desc, n_kp, k=4, return_info=True)
        assert pairs.shape == (0, 2) and pairs.dtype == np.int32 and set(info) == keys
        assert info["vocab"].ndim == 2 and info["vocab"].shape[1] == 32
        assert info["vocab"].dtype == np.uint8
        assert info["words"].shape == desc.shape[:2] and (info["words"] == -1).all()
        assert info["neighbours"].shape == (len(desc), 4) and (info["neighbours"] == -1).all()
        assert retrieval.select_pairs(desc, n_kp).shape == (0, 2)
    with pytest.raises(ValueError, match="128.*32"):
        retrieval.select_pairs(np.zeros((3, 8, 64), np.uint8), np.full(3, 8, np.int32))


def test_reconstruct_with_retrieval_on_binary_descriptors():
    """All pairs against pairs="retrieval" with every default and with a refined 4096-word
    vocabulary.  The pair lists equal the restatement's; the model is compared with the all-pairs
    run's: the same images registered, >= 0.98 of its verified matches, a median reprojection
    error at most REPROJ_MARGIN_PX above its (test_gpu_retrieval: both runs see the same keypoints
    with sigma = 0.5 px).  Should the all-pairs baseline itself register fewer than half of the
    images, that is a finding about the Hamming driver path: registered and n_verified are then
    compared relative to the baseline only."""
    s = cases.local_scene()
    intr = np.c_[s["cams"][:, 6:8], s["pp"]]
    n = cases.SCENE_N_IMG
    full = incremental.reconstruct(s["desc"], s["kps"], s["n_kp"], intr)
    assert len(full.pairs) == n * (n - 1) // 2
    baseline_ok = 2 * int(full.registered.sum()) >= n
    m_full = _median_reprojection(full, s) if baseline_ok else float("nan")
    print(f"all pairs: registered {int(full.registered.sum())} of {n}; n_verified "
          f"{full.n_verified}; median reprojection {m_full:.4f} px")
    runs = (("defaults", None, cases.default_ref(False)),
            ("4096 words, lloyd=2", dict(cases.SCENE_PARAMS, lloyd=2), cases.local_scene_ref(2)))
    for tag, kw, r in runs:
        ret = incremental.reconstruct(s["desc"], s["kps"], s["n_kp"], intr, pairs="retrieval",
                                      retrieval=kw)
        assert ret.pairs.tobytes() == r["pairs"].tobytes()
        assert ret.timings["select_pairs"] > 0
        m_ret = _median_reprojection(ret, s) if ret.registered.any() and baseline_ok else float("nan")
        print(f"{tag}: pairs {len(ret.pairs)}; registered {int(ret.registered.sum())}; n_verified "
              f"{ret.n_verified} ({ret.n_verified / max(full.n_verified, 1):.4f}); median "
              f"reprojection {m_ret:.4f} px")
        assert (ret.registered == full.registered).all()
        assert ret.n_verified >= 0.98 * full.n_verified
        if baseline_ok:
            assert m_ret <= m_full + REPROJ_MARGIN_PX
