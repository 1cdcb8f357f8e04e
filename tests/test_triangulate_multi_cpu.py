"""CPU: the reference of sfm_triangulate_multi (tests/tri_multi_ref.py: tri_ref.run once per round
on the compacted remainder) recovers what tests/tri_multi_cases.py plants: every merged track
yields exactly its planted number of points, each within 0.1 of its truth, and the labels are the
planted partition.  This keeps the chosen inputs inside the conditions the GPU tests rely on."""
import numpy as np
import pytest

import tri_cases
import tri_multi_cases
import tri_multi_ref
import tri_ref


def check_recovered(prob, out, name):
    """The planted points and partition of prob in the outputs `out` of a multi call."""
    pts, stats, info, n_points, label = out
    np.testing.assert_array_equal(n_points, prob["n_points"], err_msg=name)
    ptr = prob["pt_ptr"]
    for t, truth in enumerate(prob["truth"]):
        grp = prob["group"][ptr[t]:ptr[t + 1]]
        lab = label[ptr[t]:ptr[t + 1]]
        slot_of = {}
        for g, X in enumerate(truth):
            d = np.linalg.norm(pts[t, :n_points[t]] - X, axis=1)
            assert d.min() < 0.1, (name, t, g, d)
            slot_of[g] = int(d.argmin())
        assert len(set(slot_of.values())) == len(truth), (name, t)
        # lost groups are numbered after the recoverable ones (tri_multi_cases.merged)
        want = np.array([slot_of.get(int(g), -1) for g in grp], np.int8)
        np.testing.assert_array_equal(lab, want, err_msg=f"{name}: track {t}")
        for r in range(n_points[t]):
            assert stats[t, r, 3] == 0 and info[t, r, 0] == int((lab == r).sum()), (name, t, r)


def check_layout(out, R, name):
    """What the spec says of the slots from n_points on."""
    pts, stats, info, n_points, label = out
    assert pts.shape[1:] == (R, 3) and stats.shape[1:] == (R, 4) and info.shape[1:] == (R, 2)
    for t, k in enumerate(n_points):
        assert not pts[t, k:].any() and not stats[t, k:, :3].any(), (name, t)
        assert np.all(info[t, k:] == [0, -1]), (name, t)
        if k < R:
            assert stats[t, k, 3] in (1.0, 4.0, 5.0), (name, t)
            assert np.all(stats[t, k + 1:, 3] == 5.0), (name, t)
    assert label.max(initial=-1) < R and label.min(initial=-1) >= -1


@pytest.fixture(scope="module")
def cases():
    return tri_multi_cases.merges()


def test_planted_merges_are_recovered(cases):
    ends = set()
    for name, prob, kw in cases:
        tab = tri_ref.cam_table(prob["cams"], prob["pp"])
        out = tri_multi_ref.host_loop(tab, prob, **kw)
        check_layout(out, kw["max_points"], name)
        check_recovered(prob, out, name)
        stats, n_points = out[1], out[3]
        ends.update(stats[t, k, 3] for t, k in enumerate(n_points) if k < kw["max_points"])
    assert ends == {1.0, 4.0, 5.0}


def test_round_sizes_cross_the_list_boundaries(cases):
    """Round 0 takes the larger set: the sizes the GPU test counts on to visit every list."""
    name, prob, kw = cases[0]
    tab = tri_ref.cam_table(prob["cams"], prob["pp"])
    info = tri_multi_ref.host_loop(tab, prob, **kw)[2]
    sizes = {tuple(int(c) for c in row[:, 0] if c) for row in info}
    for want in ((2, 2), (3, 2), (4, 4), (9, 8), (12, 11), (70, 66), (129, 5), (6, 5, 4), (5,)):
        assert want in sizes, (want, sizes)


def test_slot_0_is_the_single_call():
    prob = tri_cases.planted_outliers(n_tracks=300)
    tab = tri_ref.cam_table(prob["cams"], prob["pp"])
    rp, rs, rm, ri = tri_ref.run(tab, prob["pt_ptr"], prob["cam_idx"], prob["uv"], prob["pt_id"])
    for R in (1, 3):
        pts, stats, info, n_points, label = tri_multi_ref.host_loop(tab, prob, max_points=R)
        check_layout((pts, stats, info, n_points, label), R, f"R={R}")
        assert pts[:, 0].tobytes() == rp.tobytes() and stats[:, 0].tobytes() == rs.tobytes()
        assert info[:, 0].tobytes() == ri.tobytes()
        np.testing.assert_array_equal(label == 0, rm.astype(bool))
        np.testing.assert_array_equal(n_points >= 1, rs[:, 3] == 0)


def test_no_later_round():
    prob = tri_multi_cases.no_later_round()
    tab = tri_ref.cam_table(prob["cams"], prob["pp"])
    pts, stats, info, n_points, label = tri_multi_ref.host_loop(tab, prob, max_points=3)
    assert not n_points.any() and np.all(label == -1) and not pts.any()
    assert set(stats[:, 0, 3].tolist()) == {1.0, 4.0}
    assert np.all(stats[:, 1:, 3] == 5.0) and not stats[:, :, :3].any()
    assert np.all(info == [0, -1])
