"""The BA step solve's CPU oracle (oracle/ba_lm.py) and the float64 restatement (hp_ref.solve_f64)
against the 50-digit reference (hp_ref.solve_blocks) on the runs of ba_solve_cases.py: asserts
what the cases claim, measures the constants K of the GPU test (test_gpu_ba_solve_hp.py), and
shows by mutation that the checks have teeth."""
import numpy as np
import pytest

import ba_edge_cases as E
import ba_lm as L
import ba_solve_cases as C
import hp_ref


def _tracks(c):
    return np.bincount(c["pt_idx"], minlength=c["n_pt"])


def _per_cam(c):
    return np.bincount(c["cam_idx"], minlength=c["n_cam"])


def test_cases_are_what_they_claim():
    b = C.case("benign")
    assert (b["n_cam"], b["n_pt"], b["n_obs"]) == (8, 60, 240) and set(_tracks(b)) == {4}
    assert _per_cam(b).min() >= 20
    g = C.case("gn")
    assert g["fixed"].sum() == 7 + 2 * 8 and _tracks(g).min() >= 2
    assert np.all(g["blocks"]["W"][g["fixed"][g["cam_idx"]]] == 0.0)
    for name, f_lo, f_hi in (("fewview", 0.9, 1.1), ("fewview_px", 900.0, 1100.0)):
        f = C.case(name)
        assert tuple(_per_cam(f)[8:]) == (1, 2, 3, 4) and _per_cam(f)[:8].min() >= 20
        assert np.all((f["prob"]["cams"][:, 6] > f_lo) & (f["prob"]["cams"][:, 6] < f_hi))
    s = C.case("single")
    t = _tracks(s)
    assert (t == 1).sum() == 12
    assert np.all(np.linalg.matrix_rank(s["blocks"]["V"][t == 1]) == 2)
    dup = np.nonzero(t == 3)[0][-1]
    assert sorted(s["cam_idx"][s["pt_idx"] == dup]) == [3, 3, 5]
    n = C.case("narrow")
    prob, t = n["prob"], _tracks(n)
    for other, deg in ((8, 0.05), (9, 0.5)):
        sel = [p for p in np.nonzero(t == 2)[0]
               if sorted(n["cam_idx"][n["pt_idx"] == p]) == [0, other]]
        assert len(sel) == 6
        for p in sel:
            rays = []
            for c in (0, other):
                cam = prob["cams"][c]
                a = prob["pts"][p] + E._R(cam[:3]).T @ cam[3:6]      # X - C
                rays.append(a / np.linalg.norm(a))
            ang = np.degrees(np.arccos(min(1.0, rays[0] @ rays[1])))
            assert 0.8 * deg <= ang <= 1.25 * deg, (deg, ang)
    assert C.reference(next(r for r in C.RUNS if r.name == "narrow")).kappa.max() > 1e6
    k = C.case("clamp")
    U = k["blocks"]["U"]
    assert 0 < U[8, 7, 7] < 1e-6 and _per_cam(k)[8] == 4 and _per_cam(k)[9] == 0
    assert np.all(U[9] == 0) and np.all(U[:8, 7, 7] > 1e-6)
    uv = k["prob"]["uv"][k["cam_idx"] == 8] - k["prob"]["pp"][8]
    assert np.abs(uv).max() < 1.0                                      # within 1 px
    t = _tracks(k)
    assert t[0] == 0 and t[-1] == 0 and t[31] == 0 and (t == 0).sum() == 3
    z = C.case("zero")
    assert not z["blocks"]["gc"].any() and not z["blocks"]["gp"].any() and z["blocks"]["U"].any()
    for name in C.HANDMADE:
        h = C.case(name)
        assert h["n_obs"] == 0 and h["n_pt"] == 0 and h["n_cam"] == 5
        S = L.damp(h["blocks"]["U"], C.FALLBACK_LAMBDA)
        piv = L.cholesky_pivots(S)
        assert np.all(piv[[0, 1, 3, 4]] >= 8.0) and np.all(piv[2, :7] >= 8.0)
        assert piv[2, 7] == -1.0 + C.FALLBACK_LAMBDA * 1e-6            # exactly: integers and 2^-2
        assert np.abs(S[2, :7, :7] - np.diag(np.diag(S[2, :7, :7]))).max() >= 1.0
        assert h["blocks"]["gc"][2, 7] == (3.0 if name == "breakdown" else 0.0)
        M, bad = L.block_preconditioner(S)
        assert bad.tolist() == [False, False, True, False, False]
        np.testing.assert_array_equal(M[2], np.diag(1.0 / np.maximum(np.diag(S[2]), 1e-6)))
        p0 = np.einsum("cij,cj->ci", M, -h["blocks"]["gc"])
        pq = float(np.einsum("ci,cij,cj->", p0, S, p0))
        assert (pq < -1e12) if name == "breakdown" else (pq > 1.0)
    for name in C.NEGATIVE_OBS:
        run = next(r for r in C.RUNS if r.name == name)
        _, _, _, S, b = L.schur_rhs_and_precond(*C.solve_args(run))
        piv = L.cholesky_pivots(S)
        assert np.all(piv[:7] > 0) and np.all(piv[7, :7] > 0) and piv[7, 7] == -1.0 + 1e-4 * 1e-6
        assert not S[7, 7, :7].any() and not S[7, :7, 7].any()
        assert b[7, 7] == (-3.0 if name == "breakdown_obs" else 0.0)
        M, bad = L.block_preconditioner(S)
        assert bad.tolist() == [False] * 7 + [True]
        p0 = np.einsum("cij,cj->ci", M, b)
        pq = float((p0 * L.schur_matvec(L.damp(C.case(name)["blocks"]["U"], run.lam),
                                        L.point_inverse(C.case(name)["blocks"]["V"], run.lam,
                                                        np.ones(60)), C.case(name)["blocks"]["W"],
                                        C.case(name)["cam_idx"], C.case(name)["pt_idx"], p0)).sum())
        assert (pq < -1e12) if name == "breakdown_obs" else (pq > 1.0)
    s1, s2a, s2b, s3 = (C.case(n) for n in C.SHAPE_CASES)
    assert tuple(_per_cam(s1)) == E.S1_COUNTS
    for s, n_obs in ((s2a, 1536), (s2b, 1499)):
        assert s["n_cam"] == 260 and s["n_obs"] == n_obs
        assert set(E.S2_TRACKS) <= set(_tracks(s)) and tuple(_per_cam(s)[:9]) == E.S2_COUNTS
    t = _tracks(s3)
    assert s3["n_cam"] == 33 and s3["n_pt"] == C.S3_NPT and C.S3_NPT % 32 != 0
    assert tuple(_per_cam(s3)[:4]) == C.S3_COUNTS and _per_cam(s3)[4:].max() < 255
    assert set(C.S3_TRACKS) <= set(t) and t[-1] == 129 and t.min() >= 3
    assert s3["n_obs"] % 256 != 0 and np.all(np.diff(s3["pt_idx"]) >= 0)


def test_spd_margins_and_shape_lambdas():
    """Every S_cc of every run but the hand-made ones is positive definite by a margin (float64
    Cholesky pivots above 1e3 eps x its largest diagonal entry), so info[4] bit 1 = 0 is a fair
    demand; and the shape cases' λ is the smallest of 1e-3, 1e-2, 1e-1 with that margin at which
    the oracle converges to 1e-12 within the cap."""
    for run in C.RUNS:
        if run.name in C.NOT_SPD:
            continue
        m = C.spd_margin(run)
        print(f"SPD margin {run.id}: smallest pivot / largest diagonal = {m:.3g} "
              f"= {m / C.SPD_MARGIN:.3g} x 1e3 eps")
        assert m > C.SPD_MARGIN, run.id
    for name in C.SHAPE_CASES:
        chosen = None
        for lam in C.SHAPE_LAMBDAS:
            run = C._run(name, lam, tol=C.SHAPE_TOL, cap=C.SHAPE_CAP)
            _, _, info = C.oracle(run)
            ok = info[1] <= C.SHAPE_TOL and info[0] <= C.SHAPE_CAP and C.spd_margin(run) > C.SPD_MARGIN
            print(f"shape {name} λ = {lam:g}: oracle {int(info[0])} iterations, |r|/|b| {info[1]:.3g}, "
                  f"margin {C.spd_margin(run) / C.SPD_MARGIN:.3g} x 1e3 eps")
            if ok and chosen is None:
                chosen = lam
        print(f"shape {name}: λ = {chosen:g}")
        assert chosen == C.SHAPE_LAMBDA[name]


def test_reference_is_self_consistent():
    """The implicit 50-digit product against the dense 50-digit solve (separate code): δc* rounded
    to float64 leaves a residual of at most one unit u_r (its rounding moves S δc by at most
    eps |S||δc|), and δp* is the back-substitution of it to within the rounding of δc*."""
    for run in C.RUNS:
        if not run.small or run.tag:
            continue
        ref = C.reference(run)
        dc, dp = ref.solve_direct()
        rho, ur = ref.solve_residual(dc), ref.unit_residual(dc)
        print(f"reference {run.id}: rho(δc*) = {rho:.3g}, u_r = {ur:.3g}")
        assert rho <= ur
        err, nrm = ref.backsub_error(dc, dp)
        assert C._ratio(err, ref.unit_backsub(dc, nrm)) <= 1.0


def test_oracle_within_a_quarter_of_K():
    """The measurement behind K: prints the oracle's ratio per run and unit, asserts each within
    its recorded value (a quarter of K) and that the oracle passes every check of the GPU test."""
    worst = {}
    for run in C.RUNS:
        dc, dp, info = C.oracle(run)
        m = C.measure(run, dc, dp, info)
        rec = C.ORACLE_RATIO[run.id]
        print(f"oracle {run.id}: " + " ".join(f"{u}={m[u]:.3g}" for u in C.UNITS if u in m)
              + f"  rho_true={m['rho_true']:.3g} u_r={m['u_r']:.3g} iterations={int(info[0])}"
              f" flags={int(info[4])}")
        assert set(rec) == {u for u in C.UNITS if u in m}, run.id
        for u in rec:
            assert m[u] <= C.K[u] / 4, (run.id, u, m[u], rec[u])
            worst[u] = max(worst.get(u, 0.0), m[u])
        assert not C.failures(run, dc, dp, info, m, oracle_iters=int(info[0])), run.id
    print("oracle, worst per unit: " + " ".join(f"{u}={v:.3g}" for u, v in worst.items()))
    print("K: " + " ".join(f"{u}={v:.3g}" for u, v in C.K.items()))


def test_oracle_first_iterate_on_the_fallback_cases():
    """One iteration of the oracle against the 50-digit x_1 = α M b, M as the spec states it: the
    measurement behind K_FIRST; the 50-digit Cholesky finds the same camera not SPD."""
    for run in C.FIRST_RUNS:
        dc, _, info = C.oracle(run)
        r, bad = C.first_ratio(run, dc)
        print(f"oracle first iterate {run.id}: {r:.3g} units (K = {C.K_FIRST:.3g}), "
              f"fallback cameras {np.nonzero(bad)[0].tolist()}")
        assert info[0] == 1 and info[4] == C.FLAG_FALLBACK
        assert bad.tolist() == [c == (2 if run.name == "fallback" else 7) for c in range(len(bad))]
        assert r <= C.K_FIRST / 4


def _restated(run, mut=""):
    return hp_ref.solve_f64(*C.solve_args(run), max_iter=run.max_iter, tol=run.tol, mut=mut)


def test_restatement_passes_every_check():
    for run in C.RUNS:
        dc, dp, info = _restated(run)
        C.check(run, dc, dp, info, "restatement", oracle_iters=int(C.oracle(run)[2][0]))


# the runs on which each mutation is tried (it must fail a check on at least one)
MUTATION_RUNS = dict(a=("clamp@1",), b=("benign@0.0001", "S1@0.001"), c=("S2a@0.01", "S2b@0.001"),
                     d=("S2a@0.01", "S2b@0.001"), e=("benign@0.0001", "benign@1"),
                     f=("benign@0.0001", "single@0.0001"), g=("benign@0.0001", "benign@1"),
                     h=("breakdown@0.25", "breakdown_obs@0.0001"))


@pytest.mark.parametrize("mut", sorted(hp_ref.SOLVE_MUTATIONS))
def test_mutation_fails_a_check(mut):
    """Each mutation of the restatement must fail a check of the GPU test on at least one run;
    prints by how much (the worst ratio in units of K, or the exact check that fails)."""
    runs = {r.id: r for r in C.RUNS}
    found = []
    for rid in MUTATION_RUNS[mut]:
        run = runs[rid]
        dc, dp, info = _restated(run, mut)
        m = C.measure(run, dc, dp, info)
        bad = C.failures(run, dc, dp, info, m, oracle_iters=int(C.oracle(run)[2][0]))
        miss = max((m[u] / C.K[u] for u in C.UNITS if u in m and C.K[u] > 0), default=0.0)
        if bad:
            found.append(f"{rid}: worst {miss:.3g} x K; " + "; ".join(bad))
    print(f"mutation {mut} ({hp_ref.SOLVE_MUTATIONS[mut]}): " + (" | ".join(found) or "not noticed"))
    assert found
