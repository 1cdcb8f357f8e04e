"""CPU: the robust triangulation spec as tests/tri_ref.c states it (planted outliers, the pair
enumeration and sampler, agreement with the plain DLT), the C-ABI surface of
sfm_triangulate_robust and the driver's option check.  No GPU."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import recon
import sfmcore
import tri_cases
import tri_ref


@pytest.fixture(scope="module")
def planted():
    prob = tri_cases.planted_outliers()
    tab = tri_ref.cam_table(prob["cams"], prob["pp"])
    return prob, tri_ref.run(tab, prob["pt_ptr"], prob["cam_idx"], prob["uv"], prob["pt_id"])


def test_planted_outliers_are_found(planted):
    prob, (pts, stats, mask, info) = planted
    assert len(prob["pt_id"]) == 3000
    assert np.all(stats[:, 3] == 0)
    ptr = prob["pt_ptr"]
    wrong = [t for t in range(len(ptr) - 1)
             if not np.array_equal(mask[ptr[t]:ptr[t + 1]], prob["planted"][ptr[t]:ptr[t + 1]])]
    assert wrong == []
    np.testing.assert_array_equal(info[:, 0], np.add.reduceat(prob["planted"].astype(np.int64),
                                                              ptr[:-1]))
    # Bound: tri_ref's own largest distance to the truth on this case is 0.1176 (median 0.0060;
    # cameras within 30 x 20 degrees at distance 8, 0.5 px noise), doubled and rounded up.
    d = np.linalg.norm(pts - prob["pts"], axis=1)
    print("point error: max %.4f median %.4f" % (d.max(), np.median(d)))
    assert d.max() < 0.25


def test_stats_are_over_the_consensus_set(planted):
    prob, (pts, stats, mask, info) = planted
    assert np.all(stats[:, 0] < 4.0) and np.all(stats[:, 2] > 0) and np.all(stats[:, 1] > 0)
    # the mean error of a track with planted outliers is that of its inliers only (0.5 px noise)
    assert np.median(stats[:, 0]) < 1.0


def _philox(c, k):
    c, k = list(c), list(k)
    for r in range(10):
        if r > 0:
            k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
    return c


def _py_pair(h, n, max_hyp, seed, pt_id):
    if n * (n - 1) // 2 <= max_hyp:
        return [(i, j) for i in range(n) for j in range(i + 1, n)][h]
    r = _philox([h, 3, pt_id & 0xFFFFFFFF, 0x54524931], [seed & 0xFFFFFFFF, seed >> 32])
    a, b = (r[0] * n) >> 32, (r[1] * (n - 1)) >> 32
    if b >= a:
        b += 1
    return min(a, b), max(a, b)


@pytest.mark.parametrize("n,max_hyp", [(2, 64), (3, 64), (11, 64), (12, 66), (12, 64), (45, 1024),
                                       (40, 1), (513, 64), (100000, 256)])
def test_pairs_match_the_python_restatement(n, max_hyp):
    nh = tri_ref.n_hyp(n, max_hyp)
    assert nh == min(n * (n - 1) // 2, max_hyp)
    for seed, pid in ((42, 0), (42, 7), ((5 << 32) | 9, -3)):
        got = [tri_ref.pair(h, n, max_hyp, seed, pid) for h in range(nh)]
        assert got == [_py_pair(h, n, max_hyp, seed, pid) for h in range(nh)]
        assert all(0 <= i < j < n for i, j in got)
        assert got == [tri_ref.pair(h, n, max_hyp, seed, pid) for h in range(nh)]
    if n * (n - 1) // 2 > max_hyp and nh > 8:   # the key matters
        assert ([tri_ref.pair(h, n, max_hyp, 42, 0) for h in range(nh)]
                != [tri_ref.pair(h, n, max_hyp, 42, 1) for h in range(nh)])
        assert ([tri_ref.pair(h, n, max_hyp, 42, 0) for h in range(nh)]
                != [tri_ref.pair(h, n, max_hyp, 43, 0) for h in range(nh)])


def test_without_outliers_it_is_the_plain_dlt():
    import synth
    prob = synth.make_ba_problem(10, 300, obs_per_pt=5, seed=3, noise_px=0.5, perturb=0.0)
    ptr = np.r_[0, np.cumsum(np.bincount(prob["pt_idx"], minlength=300))].astype(np.int32)
    tab = tri_ref.cam_table(prob["cams"], prob["pp"])
    pts, stats, mask, info = tri_ref.run(tab, ptr, prob["cam_idx"], prob["uv"],
                                         np.arange(300, dtype=np.int32), thr=1e6)
    o, os_ = recon.triangulate(prob["cams"], prob["pp"], ptr, prob["cam_idx"], prob["uv"])
    assert np.all(stats[:, 3] == 0) and np.all(os_[:, 3] == 0) and np.all(mask == 1)
    np.testing.assert_allclose(pts, o, rtol=0, atol=1e-9)
    np.testing.assert_allclose(stats[:, :3], os_[:, :3], rtol=1e-8, atol=1e-9)


def test_edge_statuses():
    for name, prob, kw in tri_cases.edge_cases():
        tab = tri_ref.cam_table(prob["cams"], prob["pp"])
        pts, stats, mask, info = tri_ref.run(tab, prob["pt_ptr"], prob["cam_idx"], prob["uv"],
                                             prob["pt_id"], **kw)
        n = np.diff(prob["pt_ptr"])
        assert np.all(stats[n < 2, 3] == 1), name
        bad = stats[:, 3] != 0
        assert np.all(pts[bad] == 0) and np.all(stats[bad, :3] == 0), name
        assert np.all(info[bad, 0] == 0) and np.all(info[bad, 1] == -1), name
        assert np.all(mask[np.repeat(bad, n)] == 0), name
        if name in ("narrow",):
            assert np.all(stats[:, 3] == 4)
        if name == "two_view_miss":
            assert stats[:, 3].tolist() == [4, 4, 4, 4, 0]
        if name == "behind":
            assert stats[0, 3] == 0 and mask.tolist() == [0, 1, 1, 1, 1]
        if name == "repeated_camera":
            assert np.all(stats[:, 3] == 0) and info[0, 1] != 0   # pair (0, 1) has no baseline
        if name == "lengths":
            assert np.all(stats[n >= 2, 3] == 0)
            assert np.all(info[n >= 2, 0] >= 0.85 * n[n >= 2])


def test_entry_point_exported_and_validates():
    lib = sfmcore.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", sfmcore.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    for name in ("sfm_triangulate_robust", "sfm_triangulate_cam_table"):
        assert name in sfmcore.EXPORTED
        assert re.search(rf"\bT {name}\b", out)
    assert lib.sfm_version() == 5   # additive entry points
    P = sfmcore.TriangulateRobustParams
    assert P._fields_[0][0] == "struct_size" and C.sizeof(P) == 32
    good = lambda: P(C.sizeof(P), 64, 4.0, 0.9997, 42)
    arrays = [None] * 4
    outs = [None] * 4

    def call(ctx, n_cam, n_pt, prm):
        return lib.sfm_triangulate_robust(ctx, n_cam, None, None, n_pt, *arrays,
                                          C.byref(prm) if prm is not None else None, *outs)

    def refused(rc, word):
        msg = lib.sfm_last_error()
        assert rc == -1 and msg.startswith(b"sfm_triangulate_robust") and word in msg, msg

    # the checks below run before the context is used: any non-NULL handle reaches them
    fake = C.create_string_buffer(4096)
    ctx = C.cast(fake, C.c_void_p)
    refused(call(None, 0, 0, good()), b"NULL")
    refused(call(ctx, 0, 0, None), b"NULL")
    refused(call(ctx, -1, 0, good()), b"negative")
    refused(call(ctx, 0, -1, good()), b"negative")
    small = good()
    small.struct_size = C.sizeof(P) - 8
    refused(call(ctx, 0, 0, small), b"struct_size")
    for mh in (0, -1, 1025):
        prm = good()
        prm.max_hyp = mh
        refused(call(ctx, 0, 0, prm), b"max_hyp")
    prm = good()
    prm.thr = 0.0
    refused(call(ctx, 0, 0, prm), b"thr")
    prm = good()
    prm.max_cos2 = 1.5
    refused(call(ctx, 0, 0, prm), b"max_cos2")
    assert call(ctx, 0, 0, good()) == 0            # an empty batch is fine
    refused(call(ctx, 1, 1, good()), b"NULL array")
    assert lib.sfm_triangulate_cam_table(None, 0, None, None, None) == -1
    assert lib.sfm_last_error().startswith(b"sfm_triangulate_cam_table")


def test_unknown_triangulation_mode_is_refused():
    import incremental
    z = np.zeros((2, 8, 32), np.uint8)
    with pytest.raises(ValueError, match="triangulation"):
        incremental.reconstruct(z, np.zeros((2, 8, 2), np.float32), np.full(2, 8, np.int32),
                                np.zeros((2, 4)), triangulation="median")
