"""GPU: the ratio path's fused tail kernel (csrc/match_l2fr.hip l2fr_tail_kernel: row scans, ordered
survivors, mutual certificate in one block per pair) and the device-side list of flagged pairs that
the reverse scan and the final kernel stride over, against the CPU oracle, element for element, for
both rules the path serves.  Shapes the older sets do not reach: query counts around the tail
kernel's 256-query rounds, a pair without survivors, train images of 3 and 5 recovery groups, and
one call with more flagged (pair, query block) units than the fallback's grid."""
import functools
import os

import numpy as np
import pytest

import mutual_cert_cases as M
import oracle as O

pytestmark = pytest.mark.gpu

RULES = {"mutual": 1, "ratio_only": 0}


def _near(rng, row, n):
    v = row.astype(np.int64)[None, :] + rng.integers(-2, 3, size=(n, 128))
    return np.clip(v, 0, 255).astype(np.uint8)


def _gpu(ctx, data, rule, ratio, cap=None, max_dist=-1, cert=None):
    """(count, match, dist, (certified, flagged, dots)) of one call through SFM_L2_PATH=fr."""
    import torch
    desc, n_kp, pairs = data
    T = lambda a, t=None: torch.from_numpy(np.ascontiguousarray(a, t)).cuda()
    env = {"SFM_L2_PATH": "fr", "SFM_L2FR_CERT_CAP": cap, "SFM_L2FR_CERT": cert}
    old = {k: os.environ.get(k) for k in env}
    ctx.match_cert_stats(enable=True)
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        cnt, mt, dist = ctx.match_batch(T(desc), T(n_kp, np.int32), T(pairs, np.int32),
                                        cross_check=RULES[rule], ratio=ratio, max_dist=max_dist)
        stats = ctx.match_cert_stats(enable=False, read=True)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return cnt.cpu().numpy(), mt.cpu().numpy(), dist.cpu().numpy(), stats


def rounds_set(seed=21):
    """Query images 0..4 with 1, 255, 256, 257 and 1025 rows (the tail kernel takes 256 queries per
    round) against train image 5 (300 rows): every even query a noisy copy of a train row, every
    odd one random.  Image 6 (200 random rows) against image 5 has no survivor at 4/5."""
    rng = np.random.default_rng(seed)
    k = 1025
    desc = rng.integers(0, 256, size=(7, k, 128), dtype=np.uint8)
    for a in range(5):
        for q in range(0, k, 2):
            desc[a, q] = _near(rng, desc[5, (q * 7 + a) % 300], 1)[0]
    n_kp = np.array([1, 255, 256, 257, 1025, 300, 200], np.int32)
    return desc, n_kp, np.array([(a, 5) for a in range(5)] + [(6, 5), (5, 6)], np.int32)


def groups_set(seed=23):
    """Train images of 513, 768 and 1025 rows (3, 3 and 5 recovery groups, the last one of 1, 256
    and 1 rows) and query images whose rows are noisy copies of chosen train rows: (a) all in the
    last group, (b) in groups 0 and the last only, (c) in every group, with 33, 64 and 65 of them in
    one wave's two tiles of different groups, (d) one copy, of the last real row, (e) none (random
    rows).  Each layout pairs with each train image; the ranges hold 4 + 1 pairs."""
    rng = np.random.default_rng(seed)
    k = 1025
    nb = [513, 768, 1025]
    desc = rng.integers(0, 256, size=(3 + 15, k, 128), dtype=np.uint8)
    n_kp = list(nb)
    pairs = []
    na_cycle = [15, 257, 1025, 1, 300]
    for t, n in enumerate(nb):
        last0 = ((n - 1) // 256) * 256
        rows = {
            "a": [last0 + i % (n - last0) for i in range(40)],
            "b": [i % 256 for i in range(50)] + [last0 + i % (n - last0) for i in range(50)],
            "c": ([i for i in range(n) if i % 11 == 0] + [n - 1] + [i % 64 for i in range(33)] +
                  [256 + 64 + i % 64 for i in range(64)] + [512 - 64 + i % 64 for i in range(65)]),
            "d": [n - 1],
            "e": [],
        }
        for li, (name, rr) in enumerate(rows.items()):
            img = 3 + 5 * t + li
            na = na_cycle[li] if name == "e" else max(len(rr), 1)
            for q, j in enumerate(rr):
                desc[img, q] = _near(rng, desc[t, j], 1)[0]
            n_kp.append(min(na, k))
            pairs.append((img, t))
    return desc, np.array(n_kp, np.int32), np.array(pairs, np.int32)


def many_pairs_set(seed=29):
    """72 images of 64 descriptors, K = 64: 24 from two byte values, 24 from three (exact ties:
    threats and slow queries), 24 random ones holding noisy copies of their neighbour's rows
    (survivors without threats); all 2556 unordered pairs."""
    rng = np.random.default_rng(seed)
    k = 64

    def lv(n, levels):
        return (rng.integers(0, levels, size=(n, k, 128)) * (255 // (levels - 1))).astype(np.uint8)
    desc = np.concatenate([lv(24, 2), lv(24, 3), rng.integers(0, 256, size=(24, k, 128), dtype=np.uint8)])
    for i in range(49, 72):
        for q in range(0, 40, 2):
            desc[i, q] = _near(rng, desc[i - 1, q + 1], 1)[0]
    desc[3, 10:20] = desc[2, 5]
    n_kp = np.full(72, k, np.int32)
    n_kp[5], n_kp[30], n_kp[60] = 1, 33, 0
    pairs = np.array([(a, b) for a in range(72) for b in range(a + 1, 72)], np.int32)
    return desc, n_kp, pairs


SETS = {f.__name__[:-4]: functools.lru_cache(maxsize=None)(f)
        for f in (rounds_set, groups_set, many_pairs_set)}
SETS["ties"] = functools.lru_cache(maxsize=None)(M.tie_heavy_set)
SETS["planted"] = functools.lru_cache(maxsize=None)(lambda: M.planted_set()[:3])


@functools.lru_cache(maxsize=None)
def _oracle(name, rule, ratio, max_dist=-1):
    desc, n_kp, pairs = SETS[name]()
    return [O.match(desc[a, :n_kp[a]], desc[b, :n_kp[b]], 0, RULES[rule], ratio, max_dist)
            for a, b in pairs]


def _compare(got, ref, pairs, what):
    cnt, mt, dist = got[:3]
    for p, (q, t, d) in enumerate(ref):
        k = cnt[p]
        assert k == len(q), f"{what}: pair {p} {pairs[p]}: count {k} != oracle {len(q)}"
        np.testing.assert_array_equal(mt[p, :k, 0], q, err_msg=f"{what}: pair {p} queries")
        np.testing.assert_array_equal(mt[p, :k, 1], t, err_msg=f"{what}: pair {p} trains")
        np.testing.assert_array_equal(dist[p, :k], d, err_msg=f"{what}: pair {p} distances")


def _check(ctx, name, rule, ratio, cap=None, max_dist=-1, cert=None):
    data = SETS[name]()
    got = _gpu(ctx, data, rule, ratio, cap, max_dist, cert)
    _compare(got, _oracle(name, rule, ratio, max_dist), data[2], f"{name} {rule} {ratio} cap {cap}")
    return got


@pytest.mark.parametrize("ratio", [(4, 5), (65535, 1)])
@pytest.mark.parametrize("rule", list(RULES))
def test_query_rounds_and_ordered_output(ctx, rule, ratio):
    """na = 1, 255, 256, 257, 1025 and a pair without survivors: counts, order and values."""
    cnt = _check(ctx, "rounds", rule, ratio)[0]
    if ratio == (4, 5):
        assert cnt[5] == 0 and cnt[6] == 0      # S = 0
        if rule == "ratio_only":
            assert cnt[4] == 513                # survivors in every round of one pair


@pytest.mark.parametrize("ratio", [(4, 5), (65535, 1)])
@pytest.mark.parametrize("rule", list(RULES))
def test_train_images_of_three_and_five_groups(ctx, rule, ratio):
    cnt, mt, _, _ = _check(ctx, "groups", rule, ratio)
    if rule == "ratio_only" and ratio == (4, 5):
        desc, n_kp, pairs = SETS["groups"]()
        for t, n in enumerate([513, 768, 1025]):
            last0 = ((n - 1) // 256) * 256
            a, b, c, d, e = (5 * t + i for i in range(5))
            assert cnt[a] == 40 and (mt[a, :40, 1] >= last0).all()
            assert cnt[b] == 100 and set(mt[b, :100, 1] // 256) == {0, last0 // 256}
            assert set(mt[c, :cnt[c], 1] // 256) == set(range(last0 // 256 + 1))
            assert cnt[d] == 1 and tuple(mt[d, 0]) == (0, n - 1)
            assert cnt[e] == 0


@pytest.mark.parametrize("max_dist", [-1, 200000])
@pytest.mark.parametrize("ratio", [(4, 5), (65535, 1)])
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("name", ["ties", "planted"])
def test_slow_queries_inside_the_fused_kernel(ctx, name, rule, ratio, max_dist):
    _check(ctx, name, rule, ratio, max_dist=max_dist)


def test_flagged_list_mixed_all_and_none(ctx):
    """About 2 500 small pairs in one call: a cap that flags some pairs and certifies others, cap
    0 (all flagged: more units than the fallback's grid, so its blocks stride over the list more
    than once), a cap nothing exceeds, and no certificate at all."""
    n_pairs = len(SETS["many_pairs"]()[2])
    assert n_pairs * 1 > ctx.l2fr_rev_grid()    # K = 64: one query block per pair
    ratio = (65535, 1)
    certified, flagged, _ = _check(ctx, "many_pairs", "mutual", ratio, cap="64")[3]
    assert certified >= 1 and flagged >= 1 and certified + flagged == n_pairs
    assert _check(ctx, "many_pairs", "mutual", ratio, cap="0")[3][:2] == (0, n_pairs)
    assert _check(ctx, "many_pairs", "mutual", ratio, cap=str(1 << 40))[3][1] == 0
    _check(ctx, "many_pairs", "mutual", ratio, cert="0")
    _check(ctx, "many_pairs", "mutual", (4, 5), cap="0")


def test_flagged_list_state_does_not_leak_between_calls(ctx):
    """The same call twice on one context, then after a call of another shape that flags every
    pair: the list and its count start afresh each time."""
    first = _check(ctx, "many_pairs", "mutual", (65535, 1), cap="64")[3]
    assert _check(ctx, "many_pairs", "mutual", (65535, 1), cap="64")[3] == first
    _check(ctx, "ties", "mutual", (65535, 1), cap="0")
    assert _check(ctx, "many_pairs", "mutual", (65535, 1), cap="64")[3] == first
    _check(ctx, "many_pairs", "mutual", (65535, 1), cap=str(1 << 40))
    _check(ctx, "ties", "mutual", (4, 5))
