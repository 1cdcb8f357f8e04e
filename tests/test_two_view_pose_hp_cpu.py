"""CPU: the two-view pose spec (tests/pose_ref.c) against the 50-digit references of
tests/hp_ref.py on the cases of tests/pose_hp_cases.py: N, E, the poses, the cheirality vote, the
f32 keys, n_wide and the median, and the 10-step undistortion against the true inverse; the numpy
restatement hp_ref.pose_f64 and its mutations; the LAPACK measurements every K derives from.  The
kernels are compared with pose_ref.c byte for byte, and with the same references, in
test_gpu_two_view_pose_hp.py."""
import functools

import numpy as np
import pytest

import hp_ref
import pose_hp_cases as pc
import pose_ref

NAMES = pc.names()


@functools.lru_cache(maxsize=None)
def spec_outputs():
    """{case: pose_ref's outputs}, through pref_pose_batch, one batch per family."""
    out = {}
    for _, ns, deg in pc.batches():
        res = pose_ref.pose_batch(*pc.batch_args(ns), min_inliers=8, min_angle_deg=deg)
        for p, n in enumerate(ns):
            out[n] = pc.row(res, p)
    return out


def _front_keys(name):
    c, o = pc.case(name), spec_outputs()[name]
    l1, l2, key = hp_ref.score_f64(o["R"], o["t"], c["x1"], c["x2"])
    return np.sort(key[(l1 > 0) & (l2 > 0)])


def test_the_cases_are_what_they_claim():
    o = spec_outputs()
    assert len(NAMES) <= 48 and max(len(pc.case(n)["kp1"]) for n in NAMES) == 300
    assert o["rank1"]["stat"][0] == 2                       # status 2 through the batch entry
    assert o["zero_front"]["stat"][:6].tolist() == [0, 0, 0, 0, 0, 0]
    assert o["zero_front"]["median_key"] == 0 and o["zero_front"]["stat"][6] == 0
    nf = np.sort(o["tie"]["stat"][2:6])
    assert nf[-1] == nf[-2] > 0 and o["tie"]["stat"][1] == int(np.argmax(o["tie"]["stat"][2:6]))
    assert any(len(set(o[n]["stat"][2:6].tolist())) < 4 for n in ("junk8", "junk20", "junk64"))
    k = _front_keys("wide90")
    assert (k > 1.0).sum() >= 10 and (k < 1.0).sum() >= 2   # both sides of 90 degrees
    assert 1.0 < o["wide90"]["median_key"] < 2.0
    st = o["behind"]["stat"]
    assert sorted(st[2:6].tolist()) == [0, 5, 5, 40]        # behind one, behind both, in front
    assert o["depth"]["stat"][2 + o["depth"]["stat"][1]] == 100
    for n, delta in (("wk_eq", 0), ("wk_lo", 1), ("wk_hi", -1)):
        c, k = pc.case(n), _front_keys(n)
        wk = pose_ref.wide_key(c["min_angle_deg"])
        assert (k == c["key0"]).sum() == 1 and len(k) == 21
        assert int(wk.view(np.int32)) - int(c["key0"].view(np.int32)) == -delta
        assert o[n]["stat"][6] == (k > c["key0"]).sum() + (delta == 1)
    for n, cnt in (("med_even", 22), ("med_odd", 23)):
        k = _front_keys(n)
        assert len(k) == cnt and k[(cnt - 1) // 2] == k[cnt // 2] == k[(cnt - 1) // 2 - (cnt % 2)]
        assert o[n]["median_key"] == k[(cnt - 1) // 2]
    assert len(_front_keys("gen64")) == 64 and _front_keys("gen64")[31] < _front_keys("gen64")[32]
    # the fits meant to run many sweeps: lam1 ~ 0 against the trace
    for n in ("exact8", "exact15", "exact64"):
        assert pc.fit_ref(n)["lam"][0] < 1e-12 * pc.fit_ref(n)["lam"][8]


@pytest.mark.parametrize("name", NAMES)
def test_pose_ref_against_50_digits(name):
    c = pc.case(name)
    N = pose_ref.normal_matrix(c["x1"], c["x2"], c["mask"])
    pc.check(name, spec_outputs()[name], "pose_ref.c", N=N)


def test_the_reference_alone_meets_the_caps():
    """At most 2 % of a case's matches have a numerator within K_V units of zero in 50 digits, and
    none outside the two cases with a point on the baseline or at 1e5 baselines and more."""
    for name in NAMES:
        c, o = pc.case(name), spec_outputs()[name]
        if o["stat"][0] != 0 or not c["vote"]:
            continue
        n_exc = int(pc.excused_by_reference(name, pose_ref.candidates(o["E"])[:3]).sum())
        assert n_exc <= pc.EXCUSED_CAP * c["mask"].sum() and (c["loose"] or n_exc == 0), (name, n_exc)
    assert [n for n in NAMES if pc.case(n)["loose"]] == ["depth", "baseline"]


def test_lapack_ratios_behind_every_K():
    """numpy.linalg.eigh / svd and plain numpy float64 sums against the 50-digit reference over all
    cases, in the units of the assertions: the numbers pinned in pose_hp_cases.LAPACK_RATIO."""
    worst, where = {}, {}
    for name in NAMES:
        for k, v in pc.lapack_ratios(name, spec_outputs()[name]["E"]).items():
            if v > worst.get(k, -1.0):
                worst[k], where[k] = float(v), name
    rows = [r for r in pc.undistort_table() if r["exists"]]
    worst["U"] = max(r["numpy"] for r in rows)
    print("LAPACK / numpy worst ratios:", {k: (round(v, 3), where.get(k)) for k, v in worst.items()})
    for k, pinned in pc.LAPACK_RATIO.items():
        assert 0.5 * pinned <= worst[k] <= 2.0 * pinned, (k, worst[k], pinned)
    assert (pc.K_N, pc.K_E, pc.K_R, pc.K_V, pc.K_U) == tuple(
        4 * pc.LAPACK_RATIO[k] for k in ("N", "E", "R", "V", "U"))


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_passes(name):
    c = pc.case(name)
    o = hp_ref.pose_f64(c["x1"], c["x2"], c["mask"],
                        wide_key=pose_ref.wide_key(c["min_angle_deg"]))
    pc.check(name, o, "pose_f64", N=o["N"])


@pytest.mark.parametrize("mut", sorted(hp_ref.POSE_MUTATIONS))
def test_every_mutation_is_caught(mut):
    name = pc.MUTATION_CASES[mut]
    c = pc.case(name)
    o = hp_ref.pose_f64(c["x1"], c["x2"], c["mask"], mut=mut,
                        wide_key=pose_ref.wide_key(c["min_angle_deg"]))
    with pytest.raises(AssertionError) as e:
        pc.check(name, o, f"mutation {mut}", N=o["N"])
    print(f"mutation {mut} ({hp_ref.POSE_MUTATIONS[mut]}) on {name}: {str(e.value)[:160]}")


def test_undistortion_against_the_true_inverse():
    rows = pc.undistort_table()
    print("k1      position  k1 r_d^2   rho      px error   /steps  /exact")
    for r in rows:
        print(f"{r['k1']:+.3f}  {r['pos']:8s}  {r['kr2']:+.5f}  {r['rho']:.4f}  {r['px']:.3g}  "
              f"{r['steps']:.3f}  {r['exact']:.3f}")
    for r in rows:
        assert np.isfinite(r["x"]).all(), r
        assert r["steps"] <= pc.K_STEPS, r
        if r["exists"]:
            assert r["exact"] <= pc.K_U, r
    # no inverse only at the corner for k1 = -0.3 (r_d = 1.10 beyond the fold 2 / (3 sqrt(0.9)) =
    # 0.70); the spec's ten steps end there at a finite point far outside the image
    assert [(r["k1"], r["pos"]) for r in rows if not r["exists"]] == [(-0.3, "corner")]
    lost = [r for r in rows if not r["exists"]][0]
    assert 5.0 < np.abs(lost["x"]).max() < 20.0


def test_undistort_exact_inverts_the_distortion():
    import mpmath as mp
    for k1, xd in ((0.3, (0.96, 0.54)), (-0.1, (0.96, 0.54)), (-0.3, (0.48, 0.27)), (0.0, (0.3, 0.1))):
        x, rho = hp_ref.undistort_exact(xd, k1)
        with mp.workdps(hp_ref.DPS):
            s = 1 + mp.mpf(k1) * (x[0] ** 2 + x[1] ** 2)
            assert abs(x[0] * s - mp.mpf(xd[0])) < mp.mpf("1e-40")
            assert abs(x[1] * s - mp.mpf(xd[1])) < mp.mpf("1e-40")
            assert 0 <= rho < 1
    assert hp_ref.undistort_exact((0.96, 0.54), -0.3) == (None, None)


def test_shape_batches_on_the_spec():
    sb = pc.shape_batches()
    keys = ("E", "R", "t", "stat", "median_key")
    res = {k: pose_ref.pose_batch(*a, min_inliers=8) for k, a in sb.items()}
    assert res["stride"]["stat"][:, 0].tolist() == [0] * 6
    assert res["stride"]["stat"][:, 7].tolist() == [20] * 6
    assert res["kmax1"]["stat"][0, 0] == 1 and res["kmax1"]["stat"][1, 7] in (0, 1)
    assert res["kmax8"]["stat"][0].tolist()[0] == 0 and res["kmax8"]["stat"][0, 7] == 8
    assert res["kmax8192"]["stat"][:, 0].tolist() == [0, 0]
    assert res["kmax8192"]["stat"][:, 7].tolist() == [8192, 40]
    # counts and ids outside their arrays: clamped, as the kernels clamp them
    want = pose_ref.pose_batch(*pc.clamped(sb["clamps"]), min_inliers=8)
    for k in keys:
        np.testing.assert_array_equal(res["clamps"][k].view(np.uint8), want[k].view(np.uint8))
    st = res["clamps"]["stat"]
    assert st[:, 0].tolist() == [0, 2, 0, 0, 0, 0]          # count -5: no rows, E = e0, rank one
    assert st[:, 7].tolist() == [64, 0, 64, 64, 40, 32]
