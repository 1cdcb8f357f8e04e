"""A numpy restatement of the image-retrieval spec for binary (32-byte) descriptors
(include/sfmcore.h sfm_vocab_assign_hamming / sfm_vocab_majority, DESIGN.md §4.11 "Hamming"): word
assignment by Hamming distance, the k-majority round and the pipeline.  The stages after the
assignment work on word ids and are retrieval_ref's."""
import numpy as np

from retrieval_ref import (hist, idf_weights, neighbours, pair_list, sample_vocabulary,  # noqa: F401
                           vocabulary_size)

if hasattr(np, "bitwise_count"):
    popcount = np.bitwise_count
else:
    _POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)

    def popcount(a):
        return _POP8[a.view(np.uint8)].reshape(a.shape + (-1,)).sum(-1, dtype=np.uint8)


def assign(desc, n_kp, vocab):
    """(word [n_img,k_max] i32, dist [n_img,k_max] i32): nearest word by Hamming distance (bit
    count of the XOR), lowest index among equals; -1 / 0 from n_kp[i] on."""
    desc, vocab = np.ascontiguousarray(desc), np.ascontiguousarray(vocab)
    n_img, k_max = desc.shape[:2]
    word = np.full((n_img, k_max), -1, np.int32)
    dist = np.zeros((n_img, k_max), np.int32)
    v64 = vocab.view(np.uint64)                    # [n_words, 4]: a bit count does not care how
    for i in range(n_img):                         # the bytes are grouped
        n = int(n_kp[i])
        for lo in range(0, n, 256):
            x = desc[i, lo:min(n, lo + 256)].view(np.uint64)
            d = np.zeros((len(x), len(vocab)), np.int32)
            for c in range(v64.shape[1]):          # one column at a time bounds the staging
                d += popcount(x[:, c][:, None] ^ v64[:, c][None, :])
            j = np.argmin(d, axis=1)               # first occurrence: the lowest index
            word[i, lo:lo + len(x)] = j
            dist[i, lo:lo + len(x)] = d[np.arange(len(x)), j]
    return word, dist


def majority_round(vocab, desc, n_kp, word):
    """One k-majority round: bit b of word j becomes 1 if more than half of its members (rows
    q < n_kp[i] with word[i, q] == j; entries outside [0, n_words) skipped) have it set, keeps its
    old value on an exact tie, else 0.  A word without members keeps its bytes.  Bit b is bit
    b % 8 of byte b // 8."""
    vocab, desc, word = np.asarray(vocab), np.asarray(desc), np.asarray(word)
    n_words = len(vocab)
    valid = np.arange(desc.shape[1])[None, :] < np.asarray(n_kp)[:, None]
    valid &= (word >= 0) & (word < n_words)
    w = word[valid].astype(np.int64)
    bits = np.unpackbits(desc[valid], axis=1, bitorder="little").astype(np.int64)
    ones = np.zeros((n_words, 8 * desc.shape[2]), np.int64)
    np.add.at(ones, w, bits)
    cnt = np.bincount(w, minlength=n_words).astype(np.int64)[:, None]
    old = np.unpackbits(vocab, axis=1, bitorder="little").astype(np.int64)
    new = np.where(2 * ones > cnt, 1, np.where(2 * ones == cnt, old, 0)).astype(np.uint8)
    return np.packbits(new, axis=1, bitorder="little")


def select_pairs(desc, n_kp, k=32, vocab=None, n_words=65536, seed=0, lloyd=0):
    """The whole pipeline (at least two images, at least one descriptor); returns dict(pairs,
    vocab, words, hist, weight, neighbours, scores), as retrieval_ref.select_pairs does."""
    total = int(np.sum(n_kp))
    if vocab is None:
        vocab = sample_vocabulary(desc, n_kp, vocabulary_size(n_words, total), seed)
    for _ in range(lloyd):
        word, _ = assign(desc, n_kp, vocab)
        vocab = majority_round(vocab, desc, n_kp, word)
    word, _ = assign(desc, n_kp, vocab)
    h = hist(word, n_kp, len(vocab))
    wt = idf_weights(h)
    nbr, sc = neighbours(h, wt, k)
    return dict(pairs=pair_list(nbr), vocab=vocab, words=word, hist=h, weight=wt,
                neighbours=nbr, scores=sc)
