"""Shared by test_mutual_cert_logic_cpu.py and test_gpu_mutual_cert.py: the descriptor sets of the
mutual-certificate tests and a numpy restatement of the ratio path with the certificate
(csrc/match_l2fr.hip: forward records, interval test, recovery, row scans, then
l2fr_mutual_cert_kernel's bounds, owner table and threat checks, or the fallback).  No GPU here.
"""
import numpy as np

INF = np.iinfo(np.int64).max
CERT_TMAX = 2048        # csrc/match_l2fr.hip CERT_TMAX
CERT_CAP_DEFAULT = 16384  # csrc/match_l2fr.hip CERT_CAP_DEFAULT
RATIOS = [(4, 5), (1, 1), (3, 2), (65535, 1)]


def all_ordered_pairs(n_img):
    return np.array([[a, b] for a in range(n_img) for b in range(n_img) if a != b], np.int32)


def tie_heavy_set(seed=7):
    """8 ragged images (one empty, one with a single descriptor), K <= 640: descriptors from 2 or
    3 byte values (exact distance ties everywhere), duplicated rows within and across images."""
    rng = np.random.default_rng(seed)
    k = 640

    def lv(n, levels):
        return (rng.integers(0, levels, size=(n, k, 128)) * (255 // (levels - 1))).astype(np.uint8)
    desc = np.concatenate([lv(3, 2), lv(3, 3), rng.integers(0, 256, size=(2, k, 128), dtype=np.uint8)])
    desc[1, 40:60] = desc[0, 7]          # identical rows across images
    desc[0, 100] = desc[0, 7]            # and within one
    desc[4, :30] = desc[3, :30]
    desc[6, 10:20] = desc[7, 5]
    desc[7, 64:96] = desc[2, 64:96]
    n_kp = np.array([640, 599, 257, 96, 33, 1, 0, 130], np.int32)
    return desc, n_kp, all_ordered_pairs(len(n_kp))


def planted_set(seed=11):
    """Image 0 (queries) against image 1 (trains) holds the planted cross-check cases, by train
    pair; the other images (an empty one, a single descriptor, two ragged random ones) fill the
    batch.  Returns (desc, n_kp, pairs, planted) with planted = {name: (query, train, kept)} for
    the survivor each case is about (pair 0 -> 1, ratio 4/5)."""
    rng = np.random.default_rng(seed)
    k = 300
    desc = rng.integers(0, 256, size=(6, k, 128), dtype=np.uint8)
    n_kp = np.array([130, 97, 0, 1, 300, 257], np.int32)
    Q, Tr = desc[0], desc[1]

    def base():   # room for +-100 on any byte, an even number of odd bytes (even |y'|^2)
        v = rng.integers(60, 150, size=128).astype(np.int64)
        v[0] += int(v.sum() & 1)
        return v

    def put(dst, i, v, **delta):
        v = v.copy()
        for byte, dv in delta.items():
            v[int(byte[1:])] += dv
        dst[i] = v.astype(np.uint8)
    planted = {}
    # two survivors share j1 = 10, the later index nearer: the owner table takes query 20
    z = base(); put(Tr, 10, z); put(Q, 5, z, b3=6); put(Q, 20, z, b4=3)
    planted["shared_later_nearer"] = (5, 10, False)
    planted["shared_later_nearer_winner"] = (20, 10, True)
    # the same at equal distance: the lower index owns the train
    z = base(); put(Tr, 11, z); put(Q, 30, z, b3=5); put(Q, 40, z, b9=5)
    planted["shared_equal_lower_index"] = (30, 11, True)
    planted["shared_equal_higher_index"] = (40, 11, False)
    # a recovered query that fails the ratio exactly (d1 = 64, d2 = 100 with even norms:
    # 25 * 63 < 16 * 100 <= 25 * 64) but is nearer to train 12 than survivor 60 (d1 = 81)
    z = base(); put(Q, 50, z); put(Tr, 12, z, b0=8); put(Tr, 13, z, b1=10)
    put(Q, 60, z, b0=8, b5=9)
    planted["recovered_drop_nearer"] = (60, 12, False)
    # the same with a query the scan's interval test dropped (d1 = 64, d2 = 81): a threat
    z = base(); put(Tr, 14, z); put(Q, 70, z, b0=8); put(Tr, 15, z, b0=8, b1=9)
    put(Q, 75, z, b7=10)
    planted["unknown_nearer"] = (75, 14, False)
    # query 80's second-nearest train is survivor 85's j1 = 17 and beats it (1604 < 3600)
    z = base(); put(Tr, 16, z); put(Tr, 17, z, b0=40); put(Q, 80, z, b1=2); put(Q, 85, z, b0=100)
    planted["second_nearest_beats"] = (85, 17, False)
    # exact ties d(q', j) = d1 = 3600 through the threat path: q' = 90 < q = 95 takes the train ...
    z = base(); put(Tr, 18, z); put(Tr, 19, z, b0=40); put(Q, 90, z, b0=-20); put(Q, 95, z, b0=100)
    planted["tie_lower_index_threat"] = (95, 19, False)
    # ... q' = 105 > q = 100 does not
    z = base(); put(Tr, 20, z); put(Tr, 21, z, b0=40); put(Q, 105, z, b0=-20); put(Q, 100, z, b0=100)
    planted["tie_higher_index_threat"] = (100, 21, True)
    return desc, n_kp, all_ordered_pairs(len(n_kp)), planted


def _ratio_ok(d1, d2, num, den):
    d1, d2 = np.asarray(d1, np.int64), np.asarray(d2, np.int64)
    return (d2 == INF) | (den * den * d1 < num * num * np.where(d2 == INF, 0, d2))


def cert_match(A, B, ratio, cap=CERT_CAP_DEFAULT, max_dist=-1):
    """The L2 mutual + ratio rule for one pair as the ratio path with the certificate computes it.
    Returns (query_idx, train_idx, dist, info); info: flagged, dots, threats, survivors, and
    why[q] for every survivor ('kept', 'owner', 'threat', or 'fallback')."""
    num, den = ratio
    info = dict(flagged=cap <= 0, dots=0, threats=0, survivors=0, why={})
    empty = (np.zeros(0, np.int32),) * 3 + (info,)
    na, nb = len(A), len(B)
    if na == 0 or nb == 0:
        return empty
    X, Y = A.astype(np.int64) - 128, B.astype(np.int64) - 128
    dot = X @ Y.T
    An, Bn = (X * X).sum(1), (Y * Y).sum(1)
    d = An[:, None] + Bn[None, :] - 2 * dot
    e = dot - ((Bn + 1) >> 1)[None, :]            # the scan's accumulator
    es = np.sort(e, axis=1)
    e1, real2 = es[:, -1], nb >= 2
    e2 = es[:, -2] if real2 else np.full(na, -(1 << 40))
    ds = np.sort(d, axis=1)
    # forward scan: the interval test
    d1lo = np.maximum(An - 2 * e1 - 1, 0)
    d2hi = An - 2 * e2 if real2 else np.full(na, INF)
    d2lo = An - 2 * e2 - 1 if real2 else np.full(na, INF)
    drop = ~_ratio_ok(d1lo, d2hi, num, den)
    if max_dist >= 0:
        drop |= ~(d1lo < max_dist)
    slow = ~drop & (e2 == e1)
    cand = ~drop & ~slow
    # recovery: the unique train with e == e1 is the nearest neighbour, d1 from e1 and a parity
    j1 = e.argmax(1)
    d1 = An - 2 * e1 - (Bn[j1] & 1)
    assert (d1[cand] == d[cand, j1[cand]]).all() and (d1[cand] == ds[cand, 0]).all()
    passed = cand & _ratio_ok(d1, d2lo, num, den)
    straddle = cand & ~passed & _ratio_ok(d1, d2hi, num, den)
    if max_dist >= 0:
        passed &= d1 < max_dist
        straddle &= d1 < max_dist
    # exact row scans for ties in e and straddled decisions
    rows = slow | straddle
    j1 = np.where(rows, d.argmin(1), j1)
    d1 = np.where(rows, ds[:, 0], d1)
    b2 = ds[:, 1] if real2 else np.full(na, INF)
    ok = _ratio_ok(d1, b2, num, den) & ((max_dist < 0) | (d1 < max_dist))
    passed = np.where(rows, ok, passed)
    known = ~drop
    surv = np.flatnonzero(passed)
    info["survivors"] = S = len(surv)
    # the theorem's bounds
    bound = np.where(known, d2lo, An - 2 * e1 - 1)
    others = d.copy()   # d(q', j) >= bound[q'] for every train but a known query's own j1'
    others[np.flatnonzero(known), j1[known]] = INF
    assert (others.min(1) >= bound).all()

    def fallback():   # the reverse scan's decision: q is j1's lowest-index nearest query
        info["flagged"] = True
        keep = np.array([d[:, j1[q]].argmin() == q for q in surv], bool)
        info["why"] = {int(q): "fallback" for q in surv}
        return keep
    if S == 0 and cap > 0:
        return empty
    if cap <= 0:
        keep = fallback()
    else:
        T = d1[surv].max()
        threats = np.flatnonzero(bound <= T)
        info["threats"] = len(threats)
        if len(threats) > CERT_TMAX or len(threats) * S > cap:
            keep = fallback()
        else:
            owner = {}
            for q in np.flatnonzero(known):
                key = (int(d1[q]), int(q))
                if key < owner.get(int(j1[q]), (INF, 0)):
                    owner[int(j1[q])] = key
            owns = np.array([owner[int(j1[q])][1] == q for q in surv], bool)
            # threats x survivors: an exact distance wherever the bound does not already decide
            need = (bound[threats][:, None] <= d1[surv][None, :]) & (threats[:, None] != surv[None, :])
            dt = d[np.ix_(threats, j1[surv])]
            beats = need & ((dt < d1[surv][None, :]) |
                            ((dt == d1[surv][None, :]) & (threats[:, None] < surv[None, :])))
            info["dots"] = int(need.sum())
            killed = beats.any(0)
            keep = owns & ~killed
            info["why"] = {int(q): "kept" if keep[i] else ("owner" if not owns[i] else "threat")
                           for i, q in enumerate(surv)}
    q = surv[keep]
    return q.astype(np.int32), j1[q].astype(np.int32), d1[q].astype(np.int32), info
