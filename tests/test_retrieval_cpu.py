"""CPU: the numpy restatement of the image-retrieval spec (retrieval_ref.py) against plain loops,
retrieval.py's host parts against it, and the retrieval-quality condition on the 72 x 1024
local-visibility scene (truth from point_ids)."""
import numpy as np
import pytest

import retrieval
import retrieval_cases as cases
import retrieval_ref as ref


def _assign_loop(desc, n_kp, vocab):
    word = np.full(desc.shape[:2], -1, np.int32)
    dist = np.zeros(desc.shape[:2], np.int32)
    v = vocab.astype(int)
    for i in range(desc.shape[0]):
        for q in range(int(n_kp[i])):
            x = desc[i, q].astype(int)
            best, arg = None, -1
            for j in range(len(v)):
                d = int(((x - v[j]) ** 2).sum())
                if best is None or d < best:      # strict: the lowest index keeps a tie
                    best, arg = d, j
            word[i, q], dist[i, q] = arg, best
    return word, dist


def test_assign_resolves_ties_to_the_lowest_index():
    desc, n_kp, vocab = cases.tie_case(3, n_img=3, k_max=20, n_words=140)
    word, dist = ref.assign(desc, n_kp, vocab)
    w2, d2 = _assign_loop(desc, n_kp, vocab)
    assert (word == w2).all() and (dist == d2).all()
    # the case is tie-heavy: most descriptors have several nearest words
    full = ((desc[:, :, None, :].astype(int) - vocab[None, None].astype(int)) ** 2).sum(-1)
    tied = (full == full.min(-1, keepdims=True)).sum(-1) > 1
    valid = np.arange(desc.shape[1])[None, :] < n_kp[:, None]
    assert tied[valid].mean() > 0.9
    assert (word[~valid] == -1).all() and (dist[~valid] == 0).all()


def test_assign_random_and_extremes_against_the_loop():
    desc, n_kp, vocab = cases.random_case(11, 3, 12, 33)
    assert all((a == b).all() for a, b in zip(ref.assign(desc, n_kp, vocab),
                                              _assign_loop(desc, n_kp, vocab)))
    for desc, n_kp, vocab in cases.extreme_case():
        d, n = desc[:, :9], np.minimum(n_kp, 9)
        assert all((a == b).all() for a, b in zip(ref.assign(d, n, vocab),
                                                  _assign_loop(d, n, vocab)))
    # the largest distance: 128 * 255^2
    _, dist = ref.assign(np.zeros((1, 1, 128), np.uint8), [1], np.full((1, 128), 255, np.uint8))
    assert dist[0, 0] == 128 * 255 * 255


def test_hist_and_neighbours_against_stable_argsort():
    word, n_kp = cases.hist_case(4, 33, 33)
    h = ref.hist(word, n_kp, 33)
    assert h.dtype == np.uint16 and (h.sum(1) == [(word[i, :n_kp[i]] >= 0).sum()
                                                  for i in range(33)]).all()
    wt = ref.idf_weights(h)
    s = ref.scores(h, wt)
    for a in range(33):
        for b in range(33):
            assert s[a, b] == sum(min(int(h[a, w]), int(h[b, w])) * int(wt[w]) for w in range(33))
    for k in (1, 5, 32, 36):
        nbr, sc = ref.neighbours(h, wt, k)
        for a in range(33):
            row = s[a].copy()
            row[a] = 0
            order = [b for b in np.argsort(-row, kind="stable") if row[b] > 0][:k]
            assert nbr[a, :len(order)].tolist() == order and (nbr[a, len(order):] == -1).all()
            assert (sc[a, :len(order)] == row[order]).all() and (sc[a, len(order):] == 0).all()
    # identical images 0, 2 and 20: equal scores list the lower index first
    nbr, sc = ref.neighbours(h, wt, 32)
    seen = 0
    for a in range(33):
        row = list(nbr[a])
        if a not in (0, 2, 20) and 0 in row:
            assert s[a, 0] == s[a, 2] == s[a, 20]
            assert row.index(0) < row.index(2) < row.index(20)
            seen += 1
    assert seen > 0
    assert (nbr[5] == -1).all()                    # the image without descriptors
    assert not (nbr == 5).any()


def test_zero_weight_pairs_are_excluded():
    h = np.zeros((3, 4), np.uint16)
    h[0, 0], h[1, 0] = 3, 2                        # 0 and 1 share only word 0 ...
    h[1, 1], h[2, 1] = 1, 4                        # 1 and 2 share word 1
    wt = np.array([0, 5, 7, 7], np.int32)          # ... whose weight is 0
    nbr, sc = ref.neighbours(h, wt, 2)
    assert nbr.tolist() == [[-1, -1], [2, -1], [1, -1]]
    assert sc.tolist() == [[0, 0], [5, 0], [5, 0]]
    assert ref.pair_list(nbr).tolist() == [[1, 2]]


def test_sample_vocabulary_and_idf_weights_against_the_reference():
    desc, n_kp, _ = cases.random_case(2, 6, 40, 8)
    for n_words, seed in ((1, 0), (17, 3), (int(n_kp.sum()), 9)):
        v = retrieval.sample_vocabulary(desc, n_kp, n_words, seed)
        assert v.dtype == np.uint8 and v.tobytes() == ref.sample_vocabulary(desc, n_kp, n_words,
                                                                            seed).tobytes()
    rows = ref.valid_rows(desc, n_kp)
    sel = np.sort(np.random.Generator(np.random.PCG64(3)).choice(len(rows), 17, replace=False))
    assert (retrieval.sample_vocabulary(desc, n_kp, 17, 3) == rows[sel]).all()
    with pytest.raises(ValueError):
        retrieval.sample_vocabulary(desc, n_kp, int(n_kp.sum()) + 1)
    # idf: df = 0 (weight unused, floor(16 log2 n)), df = n_img (weight 0), and in between
    h = np.zeros((8, 5), np.uint16)
    h[:, 1] = 1
    h[:4, 2] = 9
    h[0, 3] = 2
    h[:3, 4] = 1
    w = retrieval.idf_weights(h)
    assert w.dtype == np.int32 and w.tobytes() == ref.idf_weights(h).tobytes()
    assert w.tolist() == [48, 0, 16, 48, int(np.floor(16 * np.log2(8 / 3)))]
    assert ((w >= 0) & (w <= 65535)).all()


def test_pair_list_and_check_pairs():
    nbr = np.array([[2, 1], [0, -1], [0, 1], [-1, -1]], np.int32)
    p = retrieval.pairs_of_neighbours(nbr)
    assert p.dtype == np.int32 and p.tolist() == [[0, 1], [0, 2], [1, 2]]
    assert p.tobytes() == ref.pair_list(nbr).tobytes()
    assert retrieval.pairs_of_neighbours(np.full((3, 2), -1)).shape == (0, 2)
    got = retrieval.check_pairs(np.array([[1, 2], [0, 3], [1, 2], [0, 1]]), 4)
    assert got.dtype == np.int32 and got.tolist() == [[0, 1], [0, 3], [1, 2]]
    for bad in ([[1, 1]], [[2, 1]], [[0, 4]], [[-1, 2]], [0, 1], [[0.0, 1.0]], [[0, 1, 2]]):
        with pytest.raises(ValueError):
            retrieval.check_pairs(np.array(bad), 4)


def test_lloyd_round_is_the_rounded_mean():
    desc, n_kp, vocab = cases.random_case(8, 4, 30, 9)
    new = ref.lloyd_round(vocab, desc, n_kp)
    word, _ = ref.assign(desc, n_kp, vocab)
    valid = np.arange(30)[None, :] < n_kp[:, None]
    for j in range(9):
        rows = desc[valid & (word == j)].astype(np.int64)
        if len(rows) == 0:
            assert (new[j] == vocab[j]).all()
        else:
            assert (new[j] == np.floor(rows.mean(0) + 0.5)).all()


def test_vocabulary_size_rule():
    for n_words, total, want in ((65536, 0, 0), (65536, 5, 1), (65536, 16384, 2048),
                                 (4096, 16384, 2048), (4096, 73728, 4096), (65536, 73728, 9216),
                                 (65536, 2048000, 65536), (1, 100, 1)):
        assert retrieval.vocabulary_size(n_words, total) == want
        assert ref.vocabulary_size(n_words, total) == want
    assert retrieval.MIN_DESC_PER_WORD == ref.MIN_DESC_PER_WORD == 8


def test_a_word_per_descriptor_selects_nothing_and_the_rule_prevents_it():
    """Why the rule exists: with every descriptor a word of its own (a vocabulary as large as the
    collection) no two histograms intersect.  The default call never builds that vocabulary."""
    s = cases.small_scene()
    total = int(s["n_kp"].sum())
    every = ref.sample_vocabulary(s["desc"], s["n_kp"], total)
    assert len(ref.select_pairs(s["desc"], s["n_kp"], vocab=every)["pairs"]) == 0
    assert len(cases.default_ref(True)["vocab"]) == total // 8 == 2048


def test_default_call_on_a_small_collection():
    """Every default (n_words 65536, k 32) on the scene's first 16 images, 16384 descriptors: the
    recall condition holds.  k >= n_img - 1 lists every image with a positive score, so the
    at-most-half part of the condition cannot apply to 16 images."""
    s = cases.small_scene()
    sel, n_pairs, s_sel, s_all, i_sel, i_all = cases.recall(s["point_ids"],
                                                            cases.default_ref(True)["pairs"])
    print(f"selected {sel} of {n_pairs}; >=60: {s_sel} of {s_all}; incidences {i_sel} of {i_all}")
    assert n_pairs == 120 and s_all > 50
    assert s_sel >= 0.99 * s_all
    assert i_sel >= 0.99 * i_all


def test_default_call_on_the_local_scene():
    """Every default on the whole 72 x 1024 scene (9216 words by the vocabulary-size rule): the
    full condition, at most half of the pairs included."""
    s = cases.local_scene()
    sel, n_pairs, s_sel, s_all, i_sel, i_all = cases.recall(s["point_ids"],
                                                            cases.default_ref(False)["pairs"])
    print(f"selected {sel} of {n_pairs}; >=60: {s_sel} of {s_all}; incidences {i_sel} of {i_all}")
    assert len(cases.default_ref(False)["vocab"]) == 9216
    assert 2 * sel <= n_pairs
    assert s_sel >= 0.99 * s_all
    assert i_sel >= 0.99 * i_all


def test_retrieval_quality_on_the_local_scene():
    """72 x 1024 local-visibility scene, n_words 4096, seed 7, k 24, no Lloyd round: at most half
    of all pairs are selected, and they hold >= 0.99 of the pairs sharing >= 60 points and >= 0.99
    of all shared-point incidences."""
    s = cases.local_scene()
    r = cases.local_scene_ref()
    n = cases.SCENE_N_IMG
    shared = cases.shared_points(s["point_ids"])
    iu = np.triu_indices(n, 1)
    sel = np.zeros((n, n), bool)
    sel[r["pairs"][:, 0], r["pairs"][:, 1]] = True
    sh, se = shared[iu], sel[iu]
    n_pairs = len(sh)
    strong = sh >= 60
    print(f"selected {se.sum()} of {n_pairs}; >=60: {(se & strong).sum()} of {strong.sum()}; "
          f">=30: {(se & (sh >= 30)).sum()} of {(sh >= 30).sum()}; "
          f"incidences {sh[se].sum()} of {sh.sum()}")
    assert n_pairs == 2556
    assert (r["pairs"][:, 0] < r["pairs"][:, 1]).all()
    assert 2 * se.sum() <= n_pairs
    assert (se & strong).sum() >= 0.99 * strong.sum()
    assert sh[se].sum() >= 0.99 * sh.sum()
