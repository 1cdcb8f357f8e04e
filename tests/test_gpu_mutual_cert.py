"""GPU: the L2 mutual + ratio rule through the forward-scan path with the mutual certificate
(csrc/match_l2fr.hip l2fr_mutual_cert_kernel) against the CPU oracle, bit for bit,
three ways: the default cap, SFM_L2FR_CERT_CAP=0 (every pair through the reverse scan + final
kernel) and a cap nothing exceeds; on the tie-heavy ragged sets and the planted cross-check cases
of mutual_cert_cases.py (restated in numpy by test_mutual_cert_logic_cpu.py)."""
import functools
import os

import numpy as np
import pytest

import mutual_cert_cases as M
import oracle as O

pytestmark = pytest.mark.gpu

WAYS = {"default": None, "fallback": "0", "certificate": str(1 << 40)}


def _setenv(k, v):
    if v is None:
        os.environ.pop(k, None)
    else:
        os.environ[k] = v


def _gpu(ctx, desc, n_kp, pairs, ratio, cap, max_dist=-1):
    """(count, match, dist, (certified, flagged, dots)) of one call with SFM_L2FR_CERT_CAP=cap."""
    import torch
    T = lambda a, t=None: torch.from_numpy(np.ascontiguousarray(a, t)).cuda()
    env = {"SFM_L2_PATH": "fr", "SFM_L2FR_CERT_CAP": cap}
    old = {k: os.environ.get(k) for k in env}
    ctx.match_cert_stats(enable=True)
    try:
        for k, v in env.items():
            _setenv(k, v)
        cnt, mt, dist = ctx.match_batch(T(desc), T(n_kp, np.int32), T(pairs, np.int32),
                                        cross_check=1, ratio=ratio, max_dist=max_dist)
        stats = ctx.match_cert_stats(enable=False, read=True)
    finally:
        for k, v in old.items():
            _setenv(k, v)
    return cnt.cpu().numpy(), mt.cpu().numpy(), dist.cpu().numpy(), stats


@functools.lru_cache(maxsize=None)
def _sets(name):
    return M.tie_heavy_set() if name == "ties" else M.planted_set()[:3]


@functools.lru_cache(maxsize=None)
def _oracle(name, ratio, max_dist=-1):
    desc, n_kp, pairs = _sets(name)
    return [O.match(desc[a, :n_kp[a]], desc[b, :n_kp[b]], 0, 1, ratio, max_dist) for a, b in pairs]


def _check(ctx, name, ratio, max_dist=-1):
    desc, n_kp, pairs = _sets(name)
    ref = _oracle(name, ratio, max_dist)
    stats = {}
    for way, cap in WAYS.items():
        cnt, mt, dist, stats[way] = _gpu(ctx, desc, n_kp, pairs, ratio, cap, max_dist)
        for p, (q, t, d) in enumerate(ref):
            k = cnt[p]
            assert k == len(q), f"{way}: pair {p} {pairs[p]}: count {k} != oracle {len(q)}"
            np.testing.assert_array_equal(mt[p, :k, 0], q)
            np.testing.assert_array_equal(mt[p, :k, 1], t)
            np.testing.assert_array_equal(dist[p, :k], d)
        assert stats[way][0] + stats[way][1] == len(pairs)
    assert stats["fallback"][0] == 0 and stats["fallback"][2] == 0
    assert stats["certificate"][1] == 0
    return stats


@pytest.mark.parametrize("ratio", M.RATIOS)
def test_tie_heavy_sets(ctx, ratio):
    stats = _check(ctx, "ties", ratio)
    if ratio == (65535, 1):   # both branches at the default cap
        certified, flagged, dots = stats["default"]
        assert certified >= 1 and flagged >= 1 and dots >= 1


def test_tie_heavy_set_with_a_distance_cap(ctx):
    _check(ctx, "ties", (4, 5), max_dist=200000)


def test_planted_cases(ctx):
    stats = _check(ctx, "planted", (4, 5))
    assert stats["default"][1] == 0 and stats["default"][2] >= 4
    # what each planted survivor comes to (pair 0 -> 1 is the batch's first pair)
    desc, n_kp, pairs, planted = M.planted_set()
    assert tuple(pairs[0]) == (0, 1)
    cnt, mt, _, _ = _gpu(ctx, desc, n_kp, pairs, (4, 5), None)
    kept = dict(zip(mt[0, :cnt[0], 0].tolist(), mt[0, :cnt[0], 1].tolist()))
    for name, (q, t, keep) in planted.items():
        assert (kept.get(q) == t) == keep, name


def test_counters_agree_with_the_restatement(ctx):
    desc, n_kp, pairs = _sets("ties")
    for ratio in [(4, 5), (65535, 1)]:
        want = [M.cert_match(desc[a, :n_kp[a]], desc[b, :n_kp[b]], ratio)[3] for a, b in pairs]
        _, _, _, (certified, flagged, dots) = _gpu(ctx, desc, n_kp, pairs, ratio, None)
        assert flagged == sum(i["flagged"] for i in want)
        assert dots == sum(i["dots"] for i in want)


def test_bench_scene_sample_is_certified_without_exact_dots(ctx):
    import synth
    s = synth.make_scene(6, 512, seed=0)
    pairs = synth.unordered_pairs(6)
    cnt, mt, dist, (certified, flagged, dots) = _gpu(ctx, s["desc"], s["n_kp"], pairs, (4, 5), None)
    assert (certified, flagged, dots) == (len(pairs), 0, 0)
    for p, (a, b) in enumerate(pairs):
        q, t, d = O.match(s["desc"][a, :s["n_kp"][a]], s["desc"][b, :s["n_kp"][b]], 0, 1, (4, 5))
        k = cnt[p]
        assert k == len(q) and (mt[p, :k, 0] == q).all() and (mt[p, :k, 1] == t).all()
        assert (dist[p, :k] == d).all()
