"""CPU: the float64 restatements (oracle/ba_lm.py log map and update, oracle/recon.py triangulation)
against 50-digit references (tests/hp_ref.py) on the edge cases of tests/recon_edge_cases.py.

* log map: rot_err(_angle_axis(R), R_50digit) <= 1e-12 for theta = pi -+ delta, delta from 0 to
  3e-2, and for angles from 0 to 2.5, each about e_x, e_y, e_z and 8 random axes; |r| <= pi;
* update: compositions landing at pi -+ delta against the 50-digit product of the two rotations;
* triangulation: numpy eigh against the 50-digit eigenvector, within the kappa-scaled bound; the
  worst ratio measured here is the one K in recon_edge_cases.py is derived from.
"""
import numpy as np
import pytest

import ba_lm as L
import hp_ref
import recon
import recon_edge_cases as E


def logmap_sweep(angle_axis):
    """Worst (error, label) of angle_axis over the sweep, and the largest |r| - pi."""
    worst, over = (0.0, ""), -np.inf
    for label, R, R_hp in E.logmap_cases():
        r = angle_axis(R.copy())
        worst = max(worst, (hp_ref.rot_err(r, R_hp), label))
        over = max(over, float(np.linalg.norm(r)) - np.pi)
    return worst, over


def test_log_map_sweep():
    (err, label), over = logmap_sweep(L._angle_axis)
    print(f"log map: worst |rotmat(log R) - R| = {err:.3g} at {label}; max |r| - pi = {over:.3g}")
    assert err <= E.LOGMAP_TOL, f"{err:.3g} at {label}"
    assert over <= 1e-12


def test_log_map_takes_every_column_near_pi():
    """e_x, e_y, e_z at pi - 1e-8 return that axis (each choice of the largest-diagonal column)."""
    cases = dict((label, R) for label, R, _ in E.logmap_cases())
    for i in range(3):
        r = L._angle_axis(cases[f"theta=pi-1e-08 axis#{i}"].copy())
        assert int(np.argmax(np.abs(r))) == i and abs(np.linalg.norm(r) - np.pi) < 2e-8


def test_update_at_the_half_turn():
    cams, dc, ref = E.half_turn_update()
    out, _ = L.update(cams, np.zeros((1, 3)), dc, np.zeros((1, 3)))
    errs = [hp_ref.rot_err(out[c, :3], ref[c]) for c in range(len(cams))]
    print(f"update at pi -+ delta: worst {max(errs):.3g}")
    assert max(errs) <= E.LOGMAP_TOL
    assert np.linalg.norm(out[:, :3], axis=1).max() <= np.pi + 1e-12
    np.testing.assert_array_equal(out[:, 3:], cams[:, 3:] + dc[:, 3:])


def test_update_zero_increment_keeps_r_near_pi():
    cams, dc, _ = E.half_turn_update()
    dc = dc.copy()
    dc[:, :3] = 0.0
    out, _ = L.update(cams, np.zeros((1, 3)), dc, np.zeros((1, 3)))
    np.testing.assert_array_equal(out[:, :3], cams[:, :3])


@pytest.mark.parametrize("name", E.TRI_CASES)
def test_triangulate_oracle_matches_50_digits(name):
    c = E.tri_case(name)
    pts, st = recon.triangulate(c["cams"], c["pp"], c["pt_ptr"], c["cam_idx"], c["uv"])
    worst = E.check_triangulation(name, pts, st)
    # K = 4 x the worst ratio measured with this function; another LAPACK build may round
    # differently, but not by a factor of 2
    assert worst <= 2 * E.EIGH_RATIO, (
        f"eigh ratio {worst:.3f} far above the {E.EIGH_RATIO} that K is derived from: re-measure")


def test_cases_are_what_they_claim():
    ref = E.tri_reference("narrow")
    ang = ref["stats"][:, 1].reshape(5, 64)
    for k, deg in enumerate(E.NARROW_DEG[:3]):           # noise (0.5 px ~ 0.03 deg) blurs the rest
        assert 0.3 * deg < np.median(ang[k]) < 1.2 * deg
    assert np.median(ang[4]) < 0.2
    lens = np.diff(E.tri_case("ragged")["pt_ptr"])
    assert set(E.RAGGED_LENGTHS) <= set(lens.tolist()) and lens[0] == 0 and lens[-1] == 0
    assert lens[1] == 1 and lens[-2] == 1
    st = E.tri_reference("ragged")["stats"][:, 3]
    np.testing.assert_array_equal(st == 1, lens < 2)
    used = np.unique(E.tri_case("ragged")["cam_idx"])
    assert used.max() < 152 and len(E.tri_case("ragged")["cams"]) == 160
    assert tuple(E.tri_reference("status")["stats"][:, 3].astype(int)) == E.STATUS_EXPECTED
    s3 = E.tri_reference("status")
    np.testing.assert_allclose(s3["pts"][1], [0.5, 0.0, -5.0], atol=1e-12)
    np.testing.assert_allclose(s3["stats"][1, :3], [0.0, 11.42, -5.0], atol=5e-3)
    r2 = np.sum(E.tri_case("rotmat")["cams"][:, :3] ** 2, axis=1)
    assert (r2 == 0).sum() == 2 and ((r2 > 0) & (r2 <= 1e-20)).sum() == 2 and (r2 > 1e-20).sum() == 2
