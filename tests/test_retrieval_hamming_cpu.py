"""CPU: the numpy restatement of binary-descriptor retrieval (retrieval_hamming_ref.py) against
plain Python loops, and the retrieval-quality conditions on the 72 x 1024 local-visibility scene
with ORB-like descriptors (truth from point_ids)."""
import numpy as np
import pytest

import retrieval_hamming_cases as cases
import retrieval_hamming_ref as ref


def _bits(row):
    return [(int(row[b >> 3]) >> (b & 7)) & 1 for b in range(256)]


def _assign_loop(desc, n_kp, vocab):
    word = np.full(desc.shape[:2], -1, np.int32)
    dist = np.zeros(desc.shape[:2], np.int32)
    for i in range(desc.shape[0]):
        for q in range(int(n_kp[i])):
            best, arg = None, -1
            for j in range(len(vocab)):
                d = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(desc[i, q], vocab[j]))
                if best is None or d < best:      # strict: the lowest index keeps a tie
                    best, arg = d, j
            word[i, q], dist[i, q] = arg, best
    return word, dist


def _majority_loop(vocab, desc, n_kp, word):
    out = vocab.copy()
    for j in range(len(vocab)):
        members = [desc[i, q] for i in range(desc.shape[0]) for q in range(int(n_kp[i]))
                   if word[i, q] == j]
        if not members:
            continue
        old, rows = _bits(vocab[j]), [_bits(m) for m in members]
        new = np.zeros(32, np.uint8)
        for b in range(256):
            ones = sum(r[b] for r in rows)
            bit = 1 if 2 * ones > len(rows) else (old[b] if 2 * ones == len(rows) else 0)
            new[b >> 3] |= bit << (b & 7)
        out[j] = new
    return out


def test_assign_against_the_loop_with_ties_and_extremes():
    desc, n_kp, vocab = cases.tie_case(3, n_img=3, k_max=20, n_words=140)
    word, dist = ref.assign(desc, n_kp, vocab)
    w2, d2 = _assign_loop(desc, n_kp, vocab)
    assert word.dtype == np.int32 and dist.dtype == np.int32
    assert (word == w2).all() and (dist == d2).all()
    valid = np.arange(desc.shape[1])[None, :] < n_kp[:, None]
    assert (word[~valid] == -1).all() and (dist[~valid] == 0).all()       # rows past n_kp
    assert set(dist[valid].tolist()) == {0, 1}
    desc, n_kp, vocab = cases.random_case(11, 4, 12, 33)
    assert {0, 1, 12} <= set(n_kp.tolist())
    assert all((a == b).all() for a, b in zip(ref.assign(desc, n_kp, vocab),
                                              _assign_loop(desc, n_kp, vocab)))
    for desc, n_kp, vocab in cases.extreme_case():
        d, n = desc[:, :9], np.minimum(n_kp, 9)
        got = ref.assign(d, n, vocab)
        assert all((a == b).all() for a, b in zip(got, _assign_loop(d, n, vocab)))
    assert got[1].max() == 256                    # all ones against the one all-zero word


@pytest.mark.parametrize("n_words", [1, 9])
def test_majority_round_against_the_loop(n_words):
    desc, n_kp, word, vocab = cases.majority_case(4, n_words, n_img=5, k_max=40)
    valid = (np.arange(40)[None, :] < n_kp[:, None]) & (word >= 0) & (word < n_words)
    cnt = np.bincount(word[valid], minlength=n_words)
    if n_words > 5:      # no member, one, even and odd counts; -1, out-of-range, rows past n_kp
        assert cnt[:5].tolist() == [0, 1, 2, 3, 4]
    assert (word == -1).any() and (word == n_words).any() and (n_kp < 40).any()
    new = ref.majority_round(vocab, desc, n_kp, word)
    assert new.dtype == np.uint8 and new.shape == vocab.shape
    assert (new == _majority_loop(vocab, desc, n_kp, word)).all()
    if n_words > 5:
        full = int(np.argmax(n_kp == 40))
        assert (new[0] == vocab[0]).all()                    # no member: unchanged
        assert (new[1] == desc[full, 0]).all()               # one member: that member
        # two members: their common bits, the old word's bits where they differ
        a, b = desc[full, 1], desc[full, 2]
        assert (a != b).any() and (new[2] == ((a & b) | ((a ^ b) & vocab[2]))).all()
        assert (new != vocab).any()


def test_entry_points_are_exported_and_validate_without_a_device():
    import re
    import subprocess

    import sfmcore
    lib = sfmcore.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", sfmcore.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    for name in ("sfm_vocab_assign_hamming", "sfm_vocab_majority"):
        assert name in sfmcore.EXPORTED
        assert re.search(rf"\bT {name}\b", out), name
    assert lib.sfm_vocab_assign_hamming(None, None, None, 0, 0, None, 1, None, None) == -1
    assert b"sfm_vocab_assign_hamming" in lib.sfm_last_error()
    assert lib.sfm_vocab_majority(None, None, None, 0, 0, None, None, 1, None) == -1
    assert b"sfm_vocab_majority" in lib.sfm_last_error()


def _report(tag, point_ids, pairs):
    sel, n_pairs, s_sel, s_all, i_sel, i_all = cases.recall(point_ids, pairs)
    print(f"{tag}: selected {sel} of {n_pairs}; >=60: {s_sel} of {s_all}; "
          f"incidences {i_sel} of {i_all} ({i_sel / i_all:.4f})")
    return sel, n_pairs, s_sel, s_all, i_sel, i_all


def test_quality_with_two_majority_rounds_on_the_local_scene():
    """n_words 4096, seed 7, k 24, two k-majority rounds: at most half of the 2556 pairs, >= 0.99
    of the pairs sharing >= 60 points and of the shared-point incidences.  The unrefined figure is
    printed, not asserted (the reference measured 545 / 571 and 0.9715 for it)."""
    s = cases.local_scene()
    assert s["desc"].shape == (72, 1024, 32)
    _report("lloyd=0 (not asserted)", s["point_ids"], cases.local_scene_ref(0)["pairs"])
    r = cases.local_scene_ref(2)
    sel, n_pairs, s_sel, s_all, i_sel, i_all = _report("lloyd=2", s["point_ids"], r["pairs"])
    assert n_pairs == 2556 and len(r["vocab"]) == 4096
    assert (r["pairs"][:, 0] < r["pairs"][:, 1]).all()
    assert 2 * sel <= n_pairs
    assert s_sel >= 0.99 * s_all
    assert i_sel >= 0.99 * i_all


def test_quality_with_every_default_on_the_local_scene():
    s = cases.local_scene()
    r = cases.default_ref(False)
    sel, n_pairs, s_sel, s_all, i_sel, i_all = _report("defaults", s["point_ids"], r["pairs"])
    assert len(r["vocab"]) == 9216
    assert 2 * sel <= n_pairs
    assert s_sel >= 0.99 * s_all
    assert i_sel >= 0.99 * i_all


def test_quality_with_every_default_on_a_small_collection():
    """The scene's first 16 images: k >= n_img - 1 lists every image with a positive score, so only
    the two recall conditions apply."""
    s = cases.small_scene()
    r = cases.default_ref(True)
    sel, n_pairs, s_sel, s_all, i_sel, i_all = _report("defaults, 16 images", s["point_ids"],
                                                       r["pairs"])
    assert n_pairs == 120 and len(r["vocab"]) == 2048 and r["vocab"].shape[1] == 32
    assert s_sel >= 0.99 * s_all
    assert i_sel >= 0.99 * i_all
