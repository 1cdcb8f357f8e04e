"""GPU: the ratio path's tail on packed records (csrc/match_l2fr.hip after the forward scan: class
bytes, 8-byte forward and result records of csrc/l2fr_records.h, recovery, compaction, mutual
certificate, fallback) against the CPU oracle, element for element, for both rules it serves
(mutual + ratio, ratio only) and ratios 4/5, 1/1 and 65535/1 (the last makes every query a
candidate).  Shapes: recovery ranges of 1..4 pairs plus a leftover one, ragged sizes around the
tile, group and block sizes, an empty image, single-descriptor images, per-wave candidate counts
around the 32- and 64-candidate load rounds, one tile holding every candidate of a full range,
K = 4096 with a match at (4095, 4095), the descriptor extremes, the certificate's three ways, and
one workspace reused across shapes."""
import functools
import os

import numpy as np
import pytest

import mutual_cert_cases as M
import oracle as O

pytestmark = pytest.mark.gpu

RATIOS = [(4, 5), (1, 1), (65535, 1)]
RULES = {"mutual": 1, "ratio_only": 0}
WAYS = {"default": None, "fallback": "0", "certificate": str(1 << 40)}


def _setenv(k, v):
    if v is None:
        os.environ.pop(k, None)
    else:
        os.environ[k] = v


def _gpu(ctx, data, rule, ratio, cap=None, max_dist=-1, path="fr"):
    """(count, match, dist, (certified, flagged, dots)) of one call through SFM_L2_PATH=path."""
    import torch
    desc, n_kp, pairs = data
    T = lambda a, t=None: torch.from_numpy(np.ascontiguousarray(a, t)).cuda()
    env = {"SFM_L2_PATH": path, "SFM_L2FR_CERT_CAP": cap}
    old = {k: os.environ.get(k) for k in env}
    ctx.match_cert_stats(enable=True)
    try:
        for k, v in env.items():
            _setenv(k, v)
        cnt, mt, dist = ctx.match_batch(T(desc), T(n_kp, np.int32), T(pairs, np.int32),
                                        cross_check=RULES[rule], ratio=ratio, max_dist=max_dist)
        stats = ctx.match_cert_stats(enable=False, read=True)
    finally:
        for k, v in old.items():
            _setenv(k, v)
    return cnt.cpu().numpy(), mt.cpu().numpy(), dist.cpu().numpy(), stats


def _near(rng, row, n):
    """n noisy copies of a descriptor row (each byte moved by at most 2)."""
    v = row.astype(np.int64)[None, :] + rng.integers(-2, 3, size=(n, 128))
    return np.clip(v, 0, 255).astype(np.uint8)


def ragged_set():
    """Bench-scene descriptors cut to ragged sizes.  Query images 0..5 (na = 15, 16, 17, 255, 257,
    1025) against train images 6..11 (nb = 31, 32, 33, 255, 256, 257): train image 6 + k has
    k + 1 pairs, so the recovery ranges hold 1, 2, 3, 4, 4 + 1 and 4 + 2 pairs.  Image 12 is
    empty (as query and as train), 13 and 14 hold one descriptor (no second neighbour)."""
    import synth
    s = synth.make_scene(15, 1025, seed=3)
    n_kp = np.array([15, 16, 17, 255, 257, 1025, 31, 32, 33, 255, 256, 257, 0, 1, 1], np.int32)
    pairs = [(q, 6 + k) for k in range(6) for q in range(k + 1)]
    pairs += [(0, 12), (12, 6), (13, 14), (5, 13), (13, 11)]
    return s["desc"], n_kp, np.array(pairs, np.int32)


def counts_set(seed=5):
    """Per-wave candidate counts of the recovery (wave w owns tiles 2w, 2w + 1 of a group): two
    train images of 256 random rows (one group); the queries are noisy copies of chosen train
    rows.  Image 2 puts 0 / 1 / 32 / 33 candidates on waves 0..3 of train image 0, image 3 puts
    64 / 65 / 129 / 0 on those of train image 1."""
    rng = np.random.default_rng(seed)
    k = 258
    desc = rng.integers(0, 256, size=(4, k, 128), dtype=np.uint8)

    def queries(train, per_wave):
        rows = []
        for w, n in enumerate(per_wave):
            for i in range(n):   # spread over the wave's two tiles
                rows.append(_near(rng, desc[train, 64 * w + (i * 7) % 64], 1)[0])
        return np.array(rows, np.uint8)
    qa, qb = queries(0, (0, 1, 32, 33)), queries(1, (64, 65, 129, 0))
    desc[2, :len(qa)] = qa
    desc[3, :len(qb)] = qb
    n_kp = np.array([256, 256, len(qa), len(qb)], np.int32)
    return desc, n_kp, np.array([(2, 0), (3, 1)], np.int32)


def one_tile_set(seed=9):
    """The candidate list's worst case: five query images of 1025 rows, every row a noisy copy of
    a row of tile 1 (rows 32..63) of the one train image (257 rows, so its second group holds a
    single row and no candidate): a full range of 4 pairs plus a range of 1, all candidates in
    one tile, several load rounds for one wave."""
    rng = np.random.default_rng(seed)
    k = 1025
    desc = rng.integers(0, 256, size=(6, k, 128), dtype=np.uint8)
    for a in range(1, 6):
        for q in range(k):
            desc[a, q] = _near(rng, desc[0, 32 + (q + a) % 32], 1)[0]
    n_kp = np.array([257, k, k, k, k, k], np.int32)
    return desc, n_kp, np.array([(a, 0) for a in range(1, 6)], np.int32)


def k4096_set(seed=13):
    """One pair at K = 4096 whose match is (query 4095, train 4095)."""
    rng = np.random.default_rng(seed)
    desc = rng.integers(0, 256, size=(2, 4096, 128), dtype=np.uint8)
    desc[0, 4095] = _near(rng, desc[1, 4095], 1)[0]
    return desc, np.array([4096, 4096], np.int32), np.array([(0, 1)], np.int32)


def extremes_set(seed=17):
    """All 0 against all 255 (the largest d1, ties everywhere), all 128 (x' = 0), identical
    random images (d1 = 0), and single rows of each extreme (no second neighbour)."""
    rng = np.random.default_rng(seed)
    k = 33
    desc = np.zeros((7, k, 128), np.uint8)
    desc[1] = 255
    desc[2] = 128
    desc[3] = rng.integers(0, 256, size=(k, 128), dtype=np.uint8)
    desc[4] = desc[3]
    desc[5, 0] = 255
    n_kp = np.array([k, k, k, k, k, 1, 1], np.int32)
    return desc, n_kp, M.all_ordered_pairs(7)


def ties_set():
    return M.tie_heavy_set()


def planted_set():
    return M.planted_set()[:3]


SETS = {f.__name__[:-4]: functools.lru_cache(maxsize=None)(f)
        for f in (ragged_set, counts_set, one_tile_set, k4096_set, extremes_set, ties_set,
                  planted_set)}


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


def _check(ctx, name, rule, ratio, cap=None, max_dist=-1):
    data = SETS[name]()
    got = _gpu(ctx, data, rule, ratio, cap, max_dist)
    _compare(got, _oracle(name, rule, ratio, max_dist), data[2], f"{name} {rule} {ratio}")
    return got


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("name", ["ragged", "counts", "one_tile", "extremes"])
def test_shapes_against_the_oracle(ctx, name, rule, ratio):
    _check(ctx, name, rule, ratio)


def test_counts_set_puts_the_intended_candidates_on_each_wave(ctx):
    """Every query of the counts set is a match at 4/5 (so it was a candidate), and its train lies
    in the tiles of the wave it was built for."""
    desc, n_kp, pairs = SETS["counts"]()
    cnt, mt, _, _ = _check(ctx, "counts", "ratio_only", (4, 5))
    for p, per_wave in enumerate([(0, 1, 32, 33), (64, 65, 129, 0)]):
        assert cnt[p] == n_kp[pairs[p][0]] == sum(per_wave)
        waves = mt[p, :cnt[p], 1] // 64
        assert tuple(int((waves == w).sum()) for w in range(4)) == per_wave


def test_one_tile_set_has_every_candidate_in_one_tile(ctx):
    cnt, mt, _, _ = _check(ctx, "one_tile", "ratio_only", (65535, 1))
    assert (cnt == 1025).all()
    for p in range(len(cnt)):
        assert (mt[p, :cnt[p], 1] // 32 == 1).all()


@pytest.mark.parametrize("rule", list(RULES))
def test_k4096_boundary(ctx, rule):
    cnt, mt, _, _ = _check(ctx, "k4096", rule, (4, 5))
    k = cnt[0]
    assert k >= 1 and tuple(mt[0, k - 1]) == (4095, 4095)


@pytest.mark.parametrize("max_dist", [-1, 200000])
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("name", ["ties", "planted"])
def test_certificate_ways(ctx, name, ratio, max_dist):
    """Default cap, cap 0 (every pair flagged: the device-side counts and the spilled survivor
    lists feed the reverse scan) and a cap nothing exceeds (none flagged); at 65535/1 the default
    cap gives a mix on the tie-heavy set."""
    n_pairs = len(SETS[name]()[2])
    stats = {}
    for way, cap in WAYS.items():
        stats[way] = _check(ctx, name, "mutual", ratio, cap, max_dist)[3]
        assert stats[way][0] + stats[way][1] == n_pairs
    assert stats["fallback"][0] == 0 and stats["fallback"][2] == 0
    assert stats["certificate"][1] == 0
    if name == "ties" and ratio == (65535, 1) and max_dist < 0:
        certified, flagged, dots = stats["default"]
        assert certified >= 1 and flagged >= 1 and dots >= 1


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("name", ["ties", "planted"])
def test_ratio_only_on_the_certificate_sets(ctx, name, ratio):
    _check(ctx, name, "ratio_only", ratio)
    _check(ctx, name, "ratio_only", ratio, max_dist=200000)


def test_counters_agree_with_the_restatement(ctx):
    desc, n_kp, pairs = SETS["ties"]()
    for ratio in [(4, 5), (65535, 1)]:
        want = [M.cert_match(desc[a, :n_kp[a]], desc[b, :n_kp[b]], ratio)[3] for a, b in pairs]
        _, _, _, (certified, flagged, dots) = _gpu(ctx, (desc, n_kp, pairs), "mutual", ratio)
        assert flagged == sum(i["flagged"] for i in want)
        assert dots == sum(i["dots"] for i in want)
        assert certified + flagged == len(pairs)


def test_workspace_reuse_across_shapes(ctx):
    """Two calls of different shapes on one context with a mutual-kernel call between them: the
    second call meets the first one's packed records in the reused workspace."""
    for rule in RULES:
        _check(ctx, "one_tile", rule, (65535, 1))
        data = SETS["ragged"]()
        got = _gpu(ctx, data, "mutual", (4, 5), path="mutual")
        _compare(got, _oracle("ragged", "mutual", (4, 5)), data[2], "mutual kernel")
        _check(ctx, "ragged", rule, (4, 5))
        _check(ctx, "counts", rule, (1, 1))
