"""The BA linearisation's CPU oracle (oracle/sfm_oracle_ba.c) and the float64 restatement
(hp_ref.ba_f64) against the 50-digit reference on the cases of ba_edge_cases.py: measures the
constant K of the GPU test (test_gpu_ba_hp.py), and shows by mutation that K units have teeth."""
import ctypes as C

import numpy as np
import pytest

import ba_edge_cases as E
import hp_ref
import oracle as O


def _oracle(name, loss_s):
    c = E.case(name)
    return O.ba_jtj(c["cams"], c["pp"], c["pts"], c["cam_idx"], c["pt_idx"], c["uv"], loss_s=loss_s)


def _oracle_obs(c, o, loss_s):
    ci, pi = c["cam_idx"][o], c["pt_idx"][o]
    r, Jc, Jp, w, rho = np.zeros(2), np.zeros(16), np.zeros(6), np.zeros(1), np.zeros(1)
    O.lib().oracle_ba_obs(*(O._p(np.ascontiguousarray(v)) for v in
                            (c["cams"][ci], c["pp"][ci], c["pts"][pi], c["uv"][o])),
                          C.c_double(loss_s), O._p(r), O._p(Jc), O._p(Jp), O._p(w), O._p(rho))
    return np.concatenate([Jc.reshape(2, 8), Jp.reshape(2, 3)], axis=1), rho[0]


def test_cases_are_what_they_claim():
    c = E.case("edge")
    ref, _ = E.reference("edge", 0.0)
    n = len(c["cam_idx"])
    assert n == 416 and np.all(np.diff(c["pt_idx"]) >= 0)
    per_cam = np.bincount(c["cam_idx"], minlength=len(c["cams"]))
    per_pt = np.bincount(c["pt_idx"], minlength=len(c["pts"]))
    assert per_cam[-1] == 0 and per_pt[0] == 0 and per_pt[-1] == 0 and np.sum(per_pt == 0) == 3
    rn = np.linalg.norm(c["cams"][c["cam_idx"], :3], axis=1)
    th2 = (c["cams"][:, :3] ** 2).sum(1)
    assert np.any((th2 > 0) & (th2 <= 1e-20)) and np.any((th2 > 1e-20) & (th2 < 1e-19))
    P2 = np.array([float(hp_ref.ba_obs(c["cams"][a], c["pp"][a], c["pts"][b], c["uv"][o])["P"][2])
                   for o, (a, b) in enumerate(zip(c["cam_idx"], c["pt_idx"]))])
    p = ref["res"] + c["uv"] - c["pp"][c["cam_idx"]]       # f d p
    rnorm = np.linalg.norm(ref["res"], axis=1)
    k1 = c["cams"][c["cam_idx"], 7]
    for reg, values in (("rotation", E.ROT_NORMS), ("depth", E.DEPTHS), ("distortion", E.K1S),
                        ("loss", E.RESIDUALS)):
        for v in values:
            sel = (c["regime"] == reg) & (c["value"] == v)
            assert sel.sum() >= 8, (reg, v)
            if reg == "rotation":
                np.testing.assert_allclose(rn[sel], v, rtol=1e-12, atol=0)
                axes = c["cams"][c["cam_idx"][sel], :3]
                if v > 0:
                    for i in range(3):      # the coordinate axes are among the directions
                        assert np.any((axes[:, i] != 0) & (np.delete(axes, i, 1) == 0).all(1))
            elif reg == "depth":
                np.testing.assert_allclose(P2[sel], v, rtol=1e-9)
                X = np.linalg.norm(c["pts"][c["pt_idx"][sel]], axis=1)
                t = np.linalg.norm(c["cams"][c["cam_idx"][sel], 3:6], axis=1)
                assert np.all((X >= 0.5 * max(8, v)) & (X <= 1.5 * max(8, v)))
                assert np.all((t >= 0.2 * max(8, v)) & (t <= 3.0 * max(8, v)))   # t = P - R X
            elif reg == "distortion":
                assert np.all(k1[sel] == v)
            else:
                np.testing.assert_allclose(rnorm[sel], v, rtol=1e-3)
        others = c["regime"] != reg
        if reg == "depth":
            assert np.all((P2[others] > 3.0) & (P2[others] < 13.0))
        if reg == "distortion":
            assert np.all(np.abs(k1[others]) <= 0.02)
        if reg == "loss":
            assert np.all((rnorm[others] > 1e-3) & (rnorm[others] < 5.0))
    # |p| up to 0.9 and the distortion factor stays >= 0.5, from the reference's f d p
    dist = c["regime"] == "distortion"
    fdp = np.linalg.norm(p[dist], axis=1) / c["cams"][c["cam_idx"][dist], 6]
    assert fdp.max() > 0.6                       # d |p| at |p| = 0.9, k1 = -0.3 is 0.68
    pn = np.tile(np.linspace(0.1, 0.9, 8), len(E.K1S))
    assert np.all(1.0 + np.repeat(E.K1S, 8) * pn ** 2 >= 0.5)
    iso = c["regime"] == "isolated"
    assert iso.sum() == 8
    assert np.all(per_cam[c["cam_idx"][iso]] == 1) and np.all(per_pt[c["pt_idx"][iso]] == 1)

    s1 = E.case("S1")
    assert tuple(np.bincount(s1["cam_idx"], minlength=6)) == E.S1_COUNTS
    t1 = np.bincount(s1["pt_idx"], minlength=len(s1["pts"]))
    assert t1[0] == 0 and t1[-1] == 0 and set(t1) == {0, 1, 2, 3, 4, 5}
    for name, n_obs in E.S2_NOBS.items():
        s = E.case(name)
        assert len(s["cams"]) == 260 and len(s["cam_idx"]) == n_obs
        assert np.all(np.diff(s["pt_idx"]) >= 0)
        cnt = np.bincount(s["cam_idx"], minlength=260)
        assert tuple(cnt[:9]) == E.S2_COUNTS and cnt[9:].min() >= 1 and cnt[9:].max() <= 3
        tl = np.bincount(s["pt_idx"], minlength=len(s["pts"]))
        assert set(E.S2_TRACKS) <= set(tl) and tl[0] == 0 and tl[-1] == 0
        ptr = np.concatenate([[0], np.cumsum(tl)])
        first, last = ptr[:-1], ptr[1:] - 1
        assert any(tl[q] == 150 and first[q] % 64 == 1 for q in range(len(tl)))
        assert any(tl[q] == 257 and first[q] % 64 == 63 and last[q] % 64 == 63 for q in range(len(tl)))
        assert any(tl[q] == 64 and last[q] % 256 == 255 for q in range(len(tl)))
        for q in range(len(tl)):            # no camera twice in a track
            cams_q = s["cam_idx"][ptr[q]:ptr[q + 1]]
            assert len(set(cams_q)) == len(cams_q)
    assert E.S2_NOBS["S2a"] % 256 == 0 and E.S2_NOBS["S2b"] % 64 != 0


def test_oracle_within_recorded_ratio_of_reference():
    """The measurement behind K: prints the oracle's worst ratio per case and output.  Asserts
    that each case stays within twice its recorded ratio, so that drift makes someone re-measure."""
    by_out = {}
    for name, loss_s in E.CASES:
        r = E.ratios(name, loss_s, _oracle(name, loss_s))
        print(f"oracle {name}@{loss_s:g}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items())
              + f"  worst {max(r.values()):.3f} (recorded {E.ORACLE_RATIO[(name, loss_s)]:.3f})")
        for k, v in r.items():
            by_out[k] = max(by_out.get(k, 0.0), v)
        assert max(r.values()) <= 2 * E.ORACLE_RATIO[(name, loss_s)], (name, loss_s, r)
    print("oracle, worst per output: " + " ".join(f"{k}={v:.3f}" for k, v in by_out.items()))
    print(f"K = 4 x {max(E.ORACLE_RATIO.values()):.3f} = {E.K:.3f}")


def test_oracle_jacobian_and_rho_per_observation():
    """oracle_ba_obs itself: J and rho of every edge observation within K units."""
    c = E.case("edge")
    for loss_s in E.EDGE_LOSS:
        ref, unit = E.reference("edge", loss_s)
        got = [_oracle_obs(c, o, loss_s) for o in range(len(c["cam_idx"]))]
        r = E.ratios("edge", loss_s, dict(J=np.array([g[0] for g in got]),
                                          rho=np.array([g[1] for g in got])), keys=("J", "rho"))
        print(f"oracle_ba_obs edge@{loss_s:g}: J={r['J']:.3f} rho={r['rho']:.3f}")
        assert max(r.values()) <= E.K, r


def test_restatement_matches_reference():
    """hp_ref.ba_f64 (the source of the units and of the shape cases' Jacobians) against the
    finite-difference reference: J of every edge observation, and every output, within K."""
    for loss_s in E.EDGE_LOSS:
        c = E.case("edge")
        val, _ = hp_ref.ba_f64(*E._args(c), loss_s)
        r = E.ratios("edge", loss_s, val, keys=hp_ref.BA_OUTPUTS + ("J", "rho"))
        print(f"restatement edge@{loss_s:g}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
        assert max(r.values()) <= E.K, r


MUTATIONS = dict(a="cross term 2 k1 p0 p1 with factor 1", b="one sign of -[Y]x flipped",
                 c="d/dk1 without f", d="w = 1/(1 + e/s)", e="first-order rotmat up to 1e-12",
                 f="sin/cos rounded to float32", g="last observation of the 129-camera dropped",
                 h="rho without log1p")


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_mutation_lands_outside_K(mut):
    """Each mutation of the restatement must leave K units on at least one case."""
    worst, where = 0.0, None
    for name, loss_s in E.CASES:
        c = E.case(name)
        if mut == "g":
            if not name.startswith("S2"):
                continue
            drop = int(np.nonzero(c["cam_idx"] == E.S2_COUNTS.index(129))[0][-1])
            val, _ = hp_ref.ba_f64(*E._args(c), loss_s, exact=True, drop=drop)
        else:
            val, _ = hp_ref.ba_f64(*E._args(c), loss_s, mut=mut, exact=name != "edge")
        r = E.ratios(name, loss_s, val)
        k = max(r, key=r.get)
        if r[k] > worst:
            worst, where = r[k], f"{name}@{loss_s:g} {k}"
    print(f"mutation {mut} ({MUTATIONS[mut]}): {worst / E.K:.3g} x K at {where}")
    assert worst > E.K
