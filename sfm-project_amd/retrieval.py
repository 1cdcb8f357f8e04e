"""Image retrieval for pair selection: which image pairs are worth matching.

A visual vocabulary (a sample of the collection's own descriptors, optionally refined), the
nearest word of every descriptor (the i8 MFMA kernels), per-image term frequencies
(`sfm_bow_hist`), idf weights, and for every image its `k` best neighbours by weighted histogram
intersection (`sfm_bow_neighbours`).  The pair list is the symmetric union of those neighbour
lists.  Everything is integer and exact, so the selection is a function of the descriptors and
the parameters alone: every rank of a distributed run computes the same list without a collective.

Two descriptor widths:

* 128 bytes (L2, SIFT-like): nearest word by exact squared L2 (`sfm_vocab_assign`), refinement by
  integer Lloyd rounds (the mean rounded half up).
* 32 bytes (binary, ORB): nearest word by Hamming distance (`sfm_vocab_assign_hamming`), refinement
  by k-majority rounds (`sfm_vocab_majority`: per bit the majority of a word's members, the old
  bit on an exact tie).

Everything after the assignment works on word ids and is the same for both.  Any other width is a
ValueError.

Binary descriptors want the refinement, or a vocabulary of one word per 8 descriptors (which the
defaults give: n_words = 65536 before the vocabulary-size rule).  A numpy restatement on the
72 x 1024 local-visibility scene with ORB-like descriptors (synth.make_scene(..., orb=True), 5 %
bit flips per view) measured:

    setting                                  pairs selected  pairs sharing >= 60  shared-point
                                             of 2556         points kept          incidences kept
    n_words=4096, seed=7, k=24, lloyd=0       968            545 / 571            0.9715
    same, lloyd=2 (two k-majority rounds)     952            571 / 571            0.9981
    every default (9216 words, k=32)         1273            571 / 571            0.9997
    defaults, first 16 images (2048 words)    120 / 120       78 / 78             1.0000

An unrefined sample of 4096 words loses 4.5 % of the strong pairs (a sampled word is one noisy view
of a point); two majority rounds move each word to its members' consensus and recover them.  So on
binary descriptors use lloyd=2 with a small vocabulary, or leave n_words at its default.

This module is plumbing (numpy and torch); the kernels are in csrc/retrieval.hip and
csrc/retrieval_hamming.hip.
"""
from __future__ import annotations

import time

import numpy as np

import sfmcore


def _is_tensor(x) -> bool:
    return hasattr(x, "is_cuda")


# A sampled vocabulary holds at most one word per this many valid descriptors.  A sampled word is
# its own nearest word (distance 0), so with n_words = total every descriptor is a word of its own,
# no two histograms intersect and nothing is selected.  With one word per 8 descriptors at most an
# eighth of the descriptors are their own word and even a two-view track is split over two words
# (both views sampled) with probability 1/64.  Measured on the 72 x 1024 local-visibility scene
# (k = 24, shared-point incidences in the selected pairs): one word per 2, 4 or 8 descriptors
# 100 %, per 16 99.82 %, per 32 98.5 %, per 64 96.9 % (profiles/retrieval/README.md).
MIN_DESC_PER_WORD = 8


def vocabulary_size(n_words, total):
    """The size of a sampled vocabulary: n_words, but at most total // MIN_DESC_PER_WORD (and at
    least 1) for `total` valid descriptors; 0 when there are none."""
    if total <= 0:
        return 0
    return max(1, min(int(n_words), int(total) // MIN_DESC_PER_WORD))


def sample_vocabulary(desc, n_kp, n_words, seed=0):
    """n_words distinct descriptors as the vocabulary: with the valid descriptors in image-major
    order, rows np.sort(Generator(PCG64(seed)).choice(total, n_words, replace=False)).  desc
    [n_img,k_max,D] u8 (any row width D) as a numpy array or a torch tensor; the result is of the
    same kind."""
    n_kp_h = np.asarray(n_kp.cpu() if _is_tensor(n_kp) else n_kp, np.int64)
    total = int(n_kp_h.sum())
    n_words = int(n_words)
    if n_words > total:
        raise ValueError(f"sample_vocabulary: n_words = {n_words} exceeds the {total} valid "
                         "descriptors")
    rows = np.sort(np.random.Generator(np.random.PCG64(seed)).choice(total, n_words,
                                                                     replace=False))
    start = np.concatenate([[0], np.cumsum(n_kp_h)])
    img = np.searchsorted(start, rows, side="right") - 1
    kp = rows - start[img]
    if _is_tensor(desc):
        import torch
        return desc[torch.from_numpy(img).to(desc.device),
                    torch.from_numpy(kp).to(desc.device)].contiguous()
    return np.ascontiguousarray(np.asarray(desc)[img, kp])


def refine_vocabulary(vocab, desc, n_kp, iters, device=0, chunk=32):
    """`iters` refinement rounds on device tensors, by the width of desc.

    128 bytes: integer Lloyd rounds — assign with vocab_assign, per-word int64 sums and counts, new
    word = (2 sum + cnt) // (2 cnt) per component (the mean rounded half up).
    32 bytes: k-majority rounds — assign by Hamming distance (without distances), then
    vocab_majority: per bit 1 if more than half of the word's members have it set, the old bit on
    an exact tie, else 0.

    A word with no member keeps its bytes.  Deterministic and exact.  `chunk` bounds the int64
    staging of the Lloyd rounds only."""
    import torch
    for name, t in (("vocab", vocab), ("desc", desc), ("n_kp", n_kp)):
        if not (_is_tensor(t) and t.is_cuda):
            raise TypeError(f"refine_vocabulary: {name} must be a device tensor (select_pairs "
                            "uploads numpy arrays itself)")
    ctx = sfmcore.context(device)
    n_img, n_words = desc.shape[0], vocab.shape[0]
    if desc.shape[2] == 32:
        for _ in range(int(iters)):
            word, _ = ctx.vocab_assign(desc, n_kp, vocab, with_dist=False)
            vocab = ctx.vocab_majority(desc, n_kp, word, vocab)
        return vocab
    for _ in range(int(iters)):
        word, _ = ctx.vocab_assign(desc, n_kp, vocab, with_dist=False)
        sums = torch.zeros((n_words, 128), dtype=torch.int64, device=desc.device)
        cnt = torch.zeros(n_words, dtype=torch.int64, device=desc.device)
        for i0 in range(0, n_img, chunk):   # bounded int64 staging of the descriptors
            w = word[i0:i0 + chunk].reshape(-1)
            m = w >= 0
            idx = w[m].long()
            sums.index_add_(0, idx, desc[i0:i0 + chunk].reshape(-1, 128)[m].to(torch.int64))
            cnt += torch.bincount(idx, minlength=n_words)
        den = (2 * cnt).clamp(min=1)[:, None]
        mean = torch.div(2 * sums + cnt[:, None], den, rounding_mode="floor").to(torch.uint8)
        vocab = torch.where((cnt > 0)[:, None], mean, vocab).contiguous()
    return vocab


def idf_weights(hist):
    """weight[w] = floor(16 log2(n_img / max(df[w], 1))) as int32, df[w] the number of images with
    hist[:, w] > 0; computed on the host in float64 from the df vector.  hist [n_img,n_words] u16
    as a numpy array or a torch tensor; the result is of the same kind."""
    if _is_tensor(hist):
        import torch
        df = (hist.view(torch.int16) != 0).sum(0).cpu().numpy()
    else:
        df = (np.asarray(hist) > 0).sum(0)
    n_img = hist.shape[0]
    w = np.floor(16.0 * np.log2(np.float64(n_img) / np.maximum(df, 1).astype(np.float64)))
    w = w.astype(np.int32)
    if _is_tensor(hist):
        import torch
        return torch.from_numpy(w).to(hist.device)
    return w


def pairs_of_neighbours(nbr):
    """The symmetric union {(min(a, b), max(a, b))} of neighbour lists nbr [n_img,k] (numpy, -1 =
    none) as [P,2] int32, unique and sorted a-major."""
    nbr = np.asarray(nbr)
    n = max(nbr.shape[0], 1)
    a = np.repeat(np.arange(nbr.shape[0], dtype=np.int64), nbr.shape[1])
    b = nbr.reshape(-1).astype(np.int64)
    m = b >= 0
    a, b = a[m], b[m]
    key = np.unique(np.minimum(a, b) * n + np.maximum(a, b))   # sorted keys = a-major order
    return np.stack([key // n, key % n], 1).astype(np.int32).reshape(-1, 2)


def select_pairs(desc, n_kp, k=32, vocab=None, n_words=65536, seed=0, lloyd=0, device=0,
                 return_info=False):
    """The image pairs worth matching: [P,2] int32 (a < b), unique and sorted a-major — the order
    match_graph.shard_range and the graph exchange assume.

    n_words defaults to 65536, the kernel's largest vocabulary: on the 500 x 4096 local-visibility
    scene a 4096-word vocabulary loses 20 % of the verified pairs at k = 32 and 15 % at k = 48
    (4096 features per image fill a 4096-word histogram, so the intersection of two unrelated
    images is as large as what 60 shared points add), 16384 words lose 3 %, 65536 none, for
    25 ms instead of 2 ms (profiles/retrieval/README.md).  A sampled vocabulary is never larger
    than one word per MIN_DESC_PER_WORD valid descriptors (vocabulary_size), whatever n_words
    asks for, so a small collection gets a small vocabulary; a given `vocab` is used as it is.

    Pipeline: vocabulary (`vocab` [n,D] u8 if given, else sample_vocabulary of
    vocabulary_size(n_words, valid descriptors) words; then `lloyd` refine_vocabulary rounds) ->
    vocab_assign -> bow_hist -> idf_weights -> bow_neighbours(k) -> symmetric union.  desc
    [n_img,k_max,D] u8 and n_kp [n_img] as numpy arrays or device tensors, D = 128 (L2 distance,
    Lloyd rounds) or D = 32 (binary descriptors: Hamming distance, k-majority rounds); any other
    width is a ValueError.  On binary descriptors a small unrefined vocabulary loses pairs (the
    table in the module docstring): use lloyd=2, or the default n_words.  return_info=True
    returns (pairs, info) with the vocabulary, words, histogram, weights, neighbours, scores (host
    arrays; empty ones of the same dtypes when there are fewer than two images or no descriptor)
    and per-stage seconds (each stage ends in a device sync)."""
    import torch
    dev = torch.device("cuda", device)
    ctx = sfmcore.context(device)
    T = lambda x, dt: (x.to(dev) if _is_tensor(x) else
                       torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)).contiguous()
    desc_t, n_kp_t = T(desc, np.uint8), T(n_kp, np.int32)
    if desc_t.dim() != 3 or desc_t.shape[2] not in (128, 32):
        raise ValueError("select_pairs: desc must be [n_img, k_max, 128] u8 (L2 descriptors) or "
                         "[n_img, k_max, 32] u8 (binary descriptors, Hamming distance)")
    n_img, width = desc_t.shape[0], int(desc_t.shape[2])
    tim = {}
    t0 = time.perf_counter()

    def lap(key):
        nonlocal t0
        if return_info:
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            tim[key] = t1 - t0
            t0 = t1

    total = int(n_kp_t.sum().item()) if n_img else 0
    if vocab is None:
        n_words = vocabulary_size(n_words, total)
        vocab_t = sample_vocabulary(desc_t, n_kp_t, n_words, seed) if n_words else None
    else:
        vocab_t = T(vocab, np.uint8)
    if vocab_t is None or n_img < 2:
        pairs = np.zeros((0, 2), np.int32)
        if not return_info:
            return pairs
        nw, k_max = 0 if vocab_t is None else int(vocab_t.shape[0]), int(desc_t.shape[1])
        info = dict(vocab=np.zeros((nw, width), np.uint8) if vocab_t is None
                    else vocab_t.cpu().numpy(),
                    words=np.full((n_img, k_max), -1, np.int32),
                    hist=np.zeros((n_img, nw), np.uint16), weight=np.zeros(nw, np.int32),
                    neighbours=np.full((n_img, int(k)), -1, np.int32),
                    scores=np.zeros((n_img, int(k)), np.int64), timings=tim)
        return pairs, info
    if lloyd:
        vocab_t = refine_vocabulary(vocab_t, desc_t, n_kp_t, lloyd, device)
    lap("vocabulary")
    word, _ = ctx.vocab_assign(desc_t, n_kp_t, vocab_t, with_dist=False)
    lap("assign")
    hist = ctx.bow_hist(word, n_kp_t, vocab_t.shape[0])
    lap("hist")
    weight = idf_weights(hist)
    lap("weights")
    nbr, score = ctx.bow_neighbours(hist, weight, k)
    nbr_h = nbr.cpu().numpy()
    lap("neighbours")
    pairs = pairs_of_neighbours(nbr_h)
    lap("pairs")
    if not return_info:
        return pairs
    info = dict(vocab=vocab_t.cpu().numpy(), words=word.cpu().numpy(),
                hist=hist.cpu().numpy(), weight=weight.cpu().numpy(), neighbours=nbr_h,
                scores=score.cpu().numpy(), timings=tim)
    return pairs, info


def check_pairs(pairs, n_img):
    """A caller's pair list as [P,2] int32 in sorted unique a-major order; ValueError unless it is
    an integer [P,2] array with 0 <= a < b < n_img in every row."""
    p = np.asarray(pairs.cpu() if _is_tensor(pairs) else pairs)
    if p.ndim != 2 or p.shape[1] != 2 or not np.issubdtype(p.dtype, np.integer):
        raise ValueError("pairs must be an integer array of shape [P, 2]")
    p = p.astype(np.int64)
    if len(p) and not ((p[:, 0] >= 0) & (p[:, 0] < p[:, 1]) & (p[:, 1] < n_img)).all():
        raise ValueError(f"pairs must satisfy 0 <= a < b < n_img = {n_img} in every row")
    return np.unique(p, axis=0).astype(np.int32).reshape(-1, 2)
