"""A numpy restatement of the image-retrieval spec (include/sfmcore.h "image retrieval", DESIGN.md
§4.11): word assignment, term frequencies, idf weights, neighbours, the pair list and the Lloyd
round.  Integer arithmetic throughout.  The one float32 GEMM is exact: every partial dot product
of two u8 x 128 rows is an integer <= 128 * 255^2 < 2^24."""
import numpy as np


def assign(desc, n_kp, vocab):
    """(word [n_img,k_max] i32, dist [n_img,k_max] i32): nearest word by exact squared L2, lowest
    index among equals; -1 / 0 from n_kp[i] on."""
    desc, vocab = np.asarray(desc), np.asarray(vocab)
    n_img, k_max = desc.shape[:2]
    word = np.full((n_img, k_max), -1, np.int32)
    dist = np.zeros((n_img, k_max), np.int32)
    wf = vocab.astype(np.float32)
    wn = (vocab.astype(np.int64) ** 2).sum(1)
    for i in range(n_img):
        n = int(n_kp[i])
        for lo in range(0, n, 2048):
            x = desc[i, lo:min(n, lo + 2048)]
            dot = (x.astype(np.float32) @ wf.T).astype(np.int64)
            d2 = (x.astype(np.int64) ** 2).sum(1)[:, None] + wn[None, :] - 2 * dot
            j = np.argmin(d2, axis=1)          # first occurrence: the lowest index
            word[i, lo:lo + len(x)] = j
            dist[i, lo:lo + len(x)] = d2[np.arange(len(x)), j]
    return word, dist


def hist(word, n_kp, n_words):
    word = np.asarray(word)
    out = np.zeros((word.shape[0], n_words), np.uint16)
    for i in range(word.shape[0]):
        w = word[i, :int(n_kp[i])]
        out[i] = np.bincount(w[w >= 0], minlength=n_words).astype(np.uint16)
    return out


def idf_weights(h):
    df = (np.asarray(h) > 0).sum(0)
    n_img = h.shape[0]
    return np.floor(16.0 * np.log2(np.float64(n_img) / np.maximum(df, 1).astype(np.float64))
                    ).astype(np.int32)


def scores(h, weight):
    """[n_img,n_img] int64: sum_w min(h[a,w], h[b,w]) * weight[w]."""
    h = np.asarray(h).astype(np.int64)
    w = np.asarray(weight).astype(np.int64)
    out = np.zeros((h.shape[0], h.shape[0]), np.int64)
    for a in range(h.shape[0]):
        out[a] = np.minimum(h[a][None, :], h) @ w
    return out


def neighbours(h, weight, k):
    """(nbr [n_img,k] i32 padded with -1, score [n_img,k] i64 padded with 0): per image the up-to-k
    other images with the largest positive score, descending, lower index first among equals."""
    s = scores(h, weight)
    n = s.shape[0]
    nbr = np.full((n, k), -1, np.int32)
    sc = np.zeros((n, k), np.int64)
    for a in range(n):
        row = s[a].copy()
        row[a] = 0                              # never its own neighbour
        order = np.argsort(-row, kind="stable")
        order = order[row[order] > 0][:k]
        nbr[a, :len(order)] = order
        sc[a, :len(order)] = row[order]
    return nbr, sc


def pair_list(nbr):
    nbr = np.asarray(nbr)
    out = set()
    for a in range(nbr.shape[0]):
        for b in nbr[a]:
            if b >= 0:
                out.add((min(a, int(b)), max(a, int(b))))
    return np.array(sorted(out), np.int32).reshape(-1, 2)


def valid_rows(desc, n_kp):
    return np.concatenate([np.asarray(desc)[i, :int(n_kp[i])] for i in range(len(desc))])


def sample_vocabulary(desc, n_kp, n_words, seed=0):
    rows = valid_rows(desc, n_kp)
    if n_words > len(rows):
        raise ValueError("n_words exceeds the valid descriptors")
    sel = np.sort(np.random.Generator(np.random.PCG64(seed)).choice(len(rows), n_words,
                                                                    replace=False))
    return rows[sel]


def lloyd_round(vocab, desc, n_kp):
    word, _ = assign(desc, n_kp, vocab)
    rows = valid_rows(desc, n_kp).astype(np.int64)
    w = np.concatenate([word[i, :int(n_kp[i])] for i in range(len(desc))])
    sums = np.zeros((len(vocab), 128), np.int64)
    np.add.at(sums, w, rows)
    cnt = np.bincount(w, minlength=len(vocab)).astype(np.int64)
    new = np.array(vocab, copy=True)
    m = cnt > 0
    new[m] = ((2 * sums[m] + cnt[m, None]) // (2 * cnt[m, None])).astype(np.uint8)
    return new


MIN_DESC_PER_WORD = 8   # a sampled vocabulary has at most one word per 8 valid descriptors


def vocabulary_size(n_words, total):
    return 0 if total <= 0 else max(1, min(int(n_words), total // MIN_DESC_PER_WORD))


def select_pairs(desc, n_kp, k=32, vocab=None, n_words=65536, seed=0, lloyd=0):
    """The whole pipeline (at least two images, at least one descriptor); returns dict(pairs,
    vocab, words, hist, weight, neighbours, scores)."""
    total = int(np.sum(n_kp))
    if vocab is None:
        vocab = sample_vocabulary(desc, n_kp, vocabulary_size(n_words, total), seed)
    for _ in range(lloyd):
        vocab = lloyd_round(vocab, desc, n_kp)
    word, _ = assign(desc, n_kp, vocab)
    h = hist(word, n_kp, len(vocab))
    wt = idf_weights(h)
    nbr, sc = neighbours(h, wt, k)
    return dict(pairs=pair_list(nbr), vocab=vocab, words=word, hist=h, weight=wt,
                neighbours=nbr, scores=sc)
