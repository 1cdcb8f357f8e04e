"""CPU: the mutual certificate of the L2 ratio path (csrc/match_l2fr.hip l2fr_mutual_cert_kernel,
DESIGN.md §4.1) restated in numpy — the bounds from the forward records, the owner table, the
threat checks, the cap and the fallback (mutual_cert_cases.cert_match, which also asserts the
theorem's bounds on every query) — against the oracle's mutual + ratio rule, bit for bit."""
import numpy as np
import pytest

import mutual_cert_cases as M
import oracle as O

CAPS = [M.CERT_CAP_DEFAULT, 0, 1 << 40]


def _run(desc, n_kp, pairs, ratio, cap, max_dist=-1):
    tot = dict(flagged=0, dots=0, certified=0)
    infos = []
    for a, b in pairs:
        A, B = desc[a, :n_kp[a]], desc[b, :n_kp[b]]
        q, t, d, info = M.cert_match(A, B, ratio, cap=cap, max_dist=max_dist)
        oq, ot, od = O.match(A, B, 0, 1, ratio, max_dist)
        np.testing.assert_array_equal(q, oq)
        np.testing.assert_array_equal(t, ot)
        np.testing.assert_array_equal(d, od)
        tot["flagged"] += info["flagged"]
        tot["certified"] += not info["flagged"]
        tot["dots"] += info["dots"]
        infos.append(info)
    return tot, infos


@pytest.mark.parametrize("ratio", M.RATIOS)
def test_tie_heavy_sets_match_the_oracle(ratio):
    desc, n_kp, pairs = M.tie_heavy_set()
    for cap in CAPS:
        tot, _ = _run(desc, n_kp, pairs, ratio, cap)
        if cap == 0:
            assert tot["certified"] == 0 and tot["dots"] == 0
        if cap == 1 << 40:
            assert tot["flagged"] == 0
    if ratio == (65535, 1):   # both branches at the default cap
        tot, _ = _run(desc, n_kp, pairs, ratio, M.CERT_CAP_DEFAULT)
        assert tot["flagged"] >= 1 and tot["dots"] >= 1 and tot["certified"] >= 1


def test_tie_heavy_set_with_a_distance_cap():
    desc, n_kp, pairs = M.tie_heavy_set()
    _run(desc, n_kp, pairs, (4, 5), M.CERT_CAP_DEFAULT, max_dist=200000)


def test_planted_cases_take_their_branch():
    desc, n_kp, pairs, planted = M.planted_set()
    for cap in CAPS:
        _run(desc, n_kp, pairs, (4, 5), cap)
    q, t, d, info = M.cert_match(desc[0, :n_kp[0]], desc[1, :n_kp[1]], (4, 5))
    assert not info["flagged"] and info["dots"] >= 4
    kept = dict(zip(q.tolist(), t.tolist()))
    for name, (qq, tt, keep) in planted.items():
        assert qq in info["why"], f"{name}: query {qq} is no ratio survivor"
        assert (kept.get(qq) == tt) == keep, name
    why = info["why"]
    assert why[5] == "owner" and why[40] == "owner" and why[60] == "owner"
    assert why[75] == "threat" and why[85] == "threat" and why[95] == "threat"
    assert why[100] == "kept" and why[20] == "kept" and why[30] == "kept"


def test_bench_scene_sample_needs_no_exact_dot():
    import synth
    s = synth.make_scene(6, 512, seed=0)
    tot, infos = _run(s["desc"], s["n_kp"], synth.unordered_pairs(6), (4, 5), M.CERT_CAP_DEFAULT)
    assert tot["flagged"] == 0 and tot["dots"] == 0
    assert all(i["threats"] == 0 for i in infos) and min(i["survivors"] for i in infos) > 50
