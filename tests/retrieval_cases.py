"""Case generators of the image-retrieval tests (test_retrieval_cpu.py, test_gpu_retrieval.py)."""
import functools

import numpy as np

import retrieval_ref as ref

# the retrieval-quality scene: bench.local_scene's recipe at 72 images x 1024 keypoints
SCENE_N_IMG, SCENE_K = 72, 1024
SCENE_PARAMS = dict(n_words=4096, seed=7, k=24, lloyd=0)


@functools.lru_cache(maxsize=None)
def local_scene():
    """bench.local_scene(72, 1024): n_el = 6, grid (12, 6, 120, 40), seed 21, window 1, track
    length 5."""
    import synth
    n_el = max(1, int(round((SCENE_N_IMG / 2) ** 0.5)))
    grid = (-(-SCENE_N_IMG // n_el), n_el, 120.0, 40.0)
    assert grid == (12, 6, 120.0, 40.0)
    return synth.make_scene(SCENE_N_IMG, SCENE_K, seed=21, k1_range=0.02, window=1, grid=grid,
                            track_len=5)


@functools.lru_cache(maxsize=None)
def local_scene_ref(lloyd=0):
    """The reference's select_pairs on the scene (computed once, shared, never modified)."""
    s = local_scene()
    p = dict(SCENE_PARAMS, lloyd=lloyd)
    out = ref.select_pairs(s["desc"], s["n_kp"], **p)
    for v in out.values():
        v.setflags(write=False)
    return out


SMALL_N_IMG = 16    # the small collection: the scene's first 16 images (16384 descriptors)


def small_scene():
    s = local_scene()
    return {k: s[k][:SMALL_N_IMG] for k in ("desc", "kps", "n_kp", "point_ids", "cams", "pp")}


@functools.lru_cache(maxsize=None)
def default_ref(small):
    """The reference's select_pairs with every default (n_words 65536 before the vocabulary-size
    rule, k 32, seed 0) on the small collection or on the whole scene."""
    s = small_scene() if small else local_scene()
    out = ref.select_pairs(s["desc"], s["n_kp"])
    for v in out.values():
        v.setflags(write=False)
    return out


def recall(point_ids, pairs):
    """(selected, pairs, strong selected, strong, incidences selected, incidences) against the
    truth: strong = sharing >= 60 points."""
    n = point_ids.shape[0]
    shared = shared_points(point_ids)
    iu = np.triu_indices(n, 1)
    sel = np.zeros((n, n), bool)
    sel[pairs[:, 0], pairs[:, 1]] = True
    sh, se = shared[iu], sel[iu]
    strong = sh >= 60
    return (int(se.sum()), len(sh), int((se & strong).sum()), int(strong.sum()),
            int(sh[se].sum()), int(sh.sum()))


def shared_points(point_ids):
    """[n_img,n_img] number of 3-D points two images share (truth from point_ids)."""
    n_img = point_ids.shape[0]
    n_pts = int(point_ids.max()) + 1
    vis = np.zeros((n_img, n_pts), np.int64)
    for i in range(n_img):
        ids = point_ids[i][point_ids[i] >= 0]
        vis[i, ids] = 1
    return vis @ vis.T


def ragged_n_kp(rng, n_img, k_max):
    """Ragged counts that include 0, 1 and k_max (when there are enough images)."""
    n = rng.integers(0, k_max + 1, size=n_img).astype(np.int32)
    for i, v in enumerate((0, 1, k_max)):
        if i < n_img:
            n[(3 * i + 1) % n_img] = v
    return n


def random_case(seed, n_img, k_max, n_words):
    rng = np.random.Generator(np.random.PCG64(seed))
    desc = rng.integers(0, 256, size=(n_img, k_max, 128), dtype=np.uint8)
    vocab = rng.integers(0, 256, size=(n_words, 128), dtype=np.uint8)
    n_kp = ragged_n_kp(rng, n_img, k_max)
    if n_words > 4:        # some descriptors sit exactly on / next to a word
        take = rng.integers(0, n_words, size=(n_img, k_max))
        near = rng.random((n_img, k_max)) < 0.3
        bump = rng.integers(-2, 3, size=(n_img, k_max, 128))
        d2 = np.clip(vocab[take].astype(np.int64) + bump, 0, 255).astype(np.uint8)
        desc = np.where(near[..., None], d2, desc)
    return desc, n_kp, vocab


def tie_case(seed, n_img=5, k_max=100, n_words=257):
    """Descriptors and words from 2-3 byte values, duplicated words and descriptors: most nearest
    words are tied, often across 128-word groups."""
    rng = np.random.Generator(np.random.PCG64(seed))
    vals = np.array([0, 128, 255], np.uint8)
    base = vals[rng.integers(0, 2, size=(12, 128))]
    base[6:] = vals[rng.integers(0, 3, size=(6, 128))]
    vocab = base[rng.integers(0, 12, size=n_words)]            # every word many times over
    desc = base[rng.integers(0, 12, size=(n_img, k_max))]
    flip = rng.random((n_img, k_max)) < 0.5                     # half of them one byte off a word
    pos = rng.integers(0, 128, size=(n_img, k_max))
    d = desc.copy()
    ii, kk = np.nonzero(flip)
    d[ii, kk, pos[ii, kk]] = vals[rng.integers(0, 3, size=len(ii))]
    n_kp = ragged_n_kp(rng, n_img, k_max)
    return np.ascontiguousarray(d), n_kp, np.ascontiguousarray(vocab)


def extreme_case():
    """All-0 and all-255 rows on both sides (the largest |d^2|), between ordinary rows."""
    rng = np.random.Generator(np.random.PCG64(5))
    vocab = rng.integers(0, 256, size=(33, 128), dtype=np.uint8)
    vocab[3] = 0
    vocab[17] = 255
    vocab[32] = 255
    desc = rng.integers(0, 256, size=(2, 100, 128), dtype=np.uint8)
    desc[0, ::3] = 0
    desc[0, 1::3] = 255
    desc[1, :50] = 255
    n_kp = np.array([100, 77], np.int32)
    only = np.stack([np.zeros(128, np.uint8), np.full(128, 255, np.uint8)])
    return [(desc, n_kp, vocab), (desc, n_kp, only), (desc, n_kp, only[1:]), (desc, n_kp, only[:1])]


def hist_case(seed, n_img, n_words, k_max=64):
    """Words for the hist / neighbours tests: images draw from overlapping word ranges; includes
    identical images (equal scores), an image without descriptors and -1 entries."""
    rng = np.random.Generator(np.random.PCG64(seed))
    word = np.full((n_img, k_max), -1, np.int32)
    n_kp = np.zeros(n_img, np.int32)
    for i in range(n_img):
        n = int(rng.integers(k_max // 2, k_max + 1))
        lo = (i * 7) % max(n_words, 1)
        span = max(1, min(n_words, 40))
        word[i, :n] = (lo + rng.integers(0, span, size=n)) % n_words
        n_kp[i] = n
    if n_img >= 3:
        word[2], n_kp[2] = word[0], n_kp[0]          # identical images 0 and 2
    if n_img >= 33:
        word[20], n_kp[20] = word[0], n_kp[0]        # and 20: three-way equal scores
        n_kp[5] = 0                                  # an image without descriptors
        word[5] = -1
        word[9, ::4] = -1                            # skipped entries inside the valid range
    if n_img == 2:
        n_kp[1] = 0
        word[1] = -1
    return word, n_kp
