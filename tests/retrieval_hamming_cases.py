"""Case generators of the binary-descriptor retrieval tests (test_retrieval_hamming_cpu.py,
test_gpu_retrieval_hamming.py)."""
import functools

import numpy as np

import retrieval_cases as l2cases
import retrieval_hamming_ref as ref
from retrieval_cases import ragged_n_kp, recall, shared_points  # noqa: F401

SCENE_N_IMG, SCENE_K = l2cases.SCENE_N_IMG, l2cases.SCENE_K
SCENE_PARAMS = dict(n_words=4096, seed=7, k=24)
SMALL_N_IMG = l2cases.SMALL_N_IMG


@functools.lru_cache(maxsize=None)
def local_scene():
    """retrieval_cases.local_scene's recipe with ORB-like descriptors: 32 random bytes per point,
    5 % of the bits flipped per view."""
    import synth
    return synth.make_scene(SCENE_N_IMG, SCENE_K, seed=21, k1_range=0.02, window=1,
                            grid=(12, 6, 120.0, 40.0), track_len=5, orb=True)


def small_scene():
    s = local_scene()
    return {k: s[k][:SMALL_N_IMG] for k in ("desc", "kps", "n_kp", "point_ids", "cams", "pp")}


def _frozen(out):
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def local_scene_ref(lloyd=0):
    """The restatement's select_pairs on the scene with SCENE_PARAMS (computed once, shared,
    never modified)."""
    s = local_scene()
    return _frozen(ref.select_pairs(s["desc"], s["n_kp"], lloyd=lloyd, **SCENE_PARAMS))


@functools.lru_cache(maxsize=None)
def default_ref(small):
    """The restatement's select_pairs with every default on the small collection or the scene."""
    s = small_scene() if small else local_scene()
    return _frozen(ref.select_pairs(s["desc"], s["n_kp"]))


def flip_bits(rng, rows, n_flip):
    """rows [..., 32] u8 with n_flip[...] distinct random bits flipped."""
    bits = np.unpackbits(rows, axis=-1)
    order = np.argsort(rng.random(bits.shape), axis=-1)          # a random permutation per row
    rank = np.argsort(order, axis=-1)
    return np.packbits(bits ^ (rank < np.asarray(n_flip)[..., None]).astype(np.uint8), axis=-1)


def random_case(seed, n_img, k_max, n_words):
    """Random rows; about 30 % of the descriptors sit 0-3 bit flips from a word."""
    rng = np.random.Generator(np.random.PCG64(seed))
    desc = rng.integers(0, 256, size=(n_img, k_max, 32), dtype=np.uint8)
    vocab = rng.integers(0, 256, size=(n_words, 32), dtype=np.uint8)
    n_kp = ragged_n_kp(rng, n_img, k_max)
    take = rng.integers(0, n_words, size=(n_img, k_max))
    near = rng.random((n_img, k_max)) < 0.3
    d2 = flip_bits(rng, vocab[take], rng.integers(0, 4, size=(n_img, k_max)))
    desc = np.where(near[..., None], d2, desc)
    return np.ascontiguousarray(desc), n_kp, vocab


def tie_case(seed, n_img=5, k_max=100, n_words=257):
    """Descriptors and words from a dozen base patterns, every word many times over (also in
    later 128-word groups), half of the descriptors one bit off a word: nearly every nearest word
    is tied."""
    rng = np.random.Generator(np.random.PCG64(seed))
    base = rng.integers(0, 256, size=(12, 32), dtype=np.uint8)
    vocab = base[rng.integers(0, 12, size=n_words)]
    desc = base[rng.integers(0, 12, size=(n_img, k_max))]
    desc = flip_bits(rng, desc, (rng.random((n_img, k_max)) < 0.5).astype(np.int64))
    n_kp = ragged_n_kp(rng, n_img, k_max)
    return np.ascontiguousarray(desc), n_kp, np.ascontiguousarray(vocab)


def extreme_case():
    """All-zero and all-ones rows on both sides (distance 256 is reached), between ordinary rows;
    vocabularies of one word."""
    rng = np.random.Generator(np.random.PCG64(5))
    vocab = rng.integers(0, 256, size=(33, 32), dtype=np.uint8)
    vocab[3] = 0
    vocab[17] = 255
    vocab[32] = 255
    desc = rng.integers(0, 256, size=(2, 100, 32), dtype=np.uint8)
    desc[0, ::3] = 0
    desc[0, 1::3] = 255
    desc[1, :50] = 255
    n_kp = np.array([100, 77], np.int32)
    only = np.stack([np.zeros(32, np.uint8), np.full(32, 255, np.uint8)])
    return [(desc, n_kp, vocab), (desc, n_kp, only), (desc, n_kp, only[1:]), (desc, n_kp, only[:1])]


def majority_case(seed, n_words, n_img=4, k_max=96):
    """(desc, n_kp, word, vocab) for one majority round.  Word 0 has no member (when there is more
    than one word), word 1 exactly one, word 2 two (every differing bit is an exact tie), word 3
    three, word 4 four rows made of two different pairs (ties again), the rest random; the member
    rows of a word are noisy copies of it, so all three outcomes of a bit occur.  -1 and
    out-of-range entries and rows past n_kp carry words that would change the result if counted."""
    rng = np.random.Generator(np.random.PCG64(seed))
    vocab = rng.integers(0, 256, size=(n_words, 32), dtype=np.uint8)
    n_kp = ragged_n_kp(rng, n_img, k_max)
    full = int(np.argmax(n_kp == k_max))                        # this image holds the planted rows
    word = rng.integers(min(5, n_words - 1), n_words, size=(n_img, k_max)).astype(np.int32)
    desc = flip_bits(rng, vocab[word], rng.integers(0, 120, size=(n_img, k_max)))
    word[:, 11::5] = -1                                          # skipped entries, in every image
    word[:, 12::7] = n_words                                     # out of range above
    word[:, 13::6] = -7
    if n_words > 5:
        planted = [1, 2, 2, 3, 3, 3, 4, 4, 4, 4]
        word[full, :len(planted)] = planted
        desc[full, :len(planted)] = flip_bits(rng, vocab[planted], np.full(len(planted), 60))
        desc[full, 8], desc[full, 9] = desc[full, 6], desc[full, 7]   # word 4: two pairs
    return np.ascontiguousarray(desc), n_kp, word, vocab
