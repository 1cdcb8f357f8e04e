"""GPU: the BA step solve (sfm_ba_solve) against the 50-digit reference on the runs of
ba_solve_cases.py, through every form of the call: the implicit solve, chunk mode with 8 and with
3 chunks, and the explicit reduced camera system (8 chunks) where the case has observations.  The
blocks are the oracle's float64 linearisation (or hand-made) uploaded as they are, so the solve is
checked on exactly the reference's inputs.  Checks (ba_solve_cases.failures): every point's dp
within K u_p of the back-substitution of the kernel's own dc; exact zeros; info[1] within K u_r of
the 50-digit residual of dc; a solve that stopped early reached tol; the cap; the model terms;
δ* on the small cases; the flags of info[4]; and two calls bit-identical.  K and the units:
ba_solve_cases.py."""
import numpy as np
import pytest

import ba_solve_cases as C
import reconstruction as R

pytestmark = pytest.mark.gpu

PARAMS = [(r, m) for r in C.RUNS for m in C.MODES
          if not (m == "explicit8" and r.name in C.HANDMADE)]
_problems, _worst = {}, {}


def _problem(name, mode):
    """(BAProblem, the case's blocks on the device, after sfm_ba_fix_params for "gn"), once per
    process.  The solve reads no pp or uv: zeros stand in."""
    if (name, mode) in _problems:
        return _problems[name, mode]
    import torch
    c = C.case(name)
    chunks = dict(implicit=None, chunks8=8, chunks3=3, explicit8=8)[mode]
    P = R.BAProblem(np.zeros((c["n_cam"], 2)), c["cam_idx"], c["pt_idx"], np.zeros((c["n_obs"], 2)),
                    c["n_cam"], c["n_pt"], chunks=chunks)
    if mode == "explicit8":
        P.set_schur()
        assert P.schur.n_slot > 0
    lin = {k: torch.from_numpy(np.array(v)).cuda() for k, v in c["raw"].items()}
    if c["fixed"] is not None:
        P.ctx.ba_fix_params(lin, P.cam_idx, torch.from_numpy(c["fixed"].astype(np.uint8)).cuda())
        for k, v in c["blocks"].items():          # the reference's inputs, bit for bit
            np.testing.assert_array_equal(lin[k].cpu().numpy(), v, err_msg=k)
    _problems[name, mode] = (P, lin)
    return P, lin


def _solve(run, mode):
    import torch
    P, lin = _problem(run.name, mode)
    out = P.solve(lin, run.lam, max_iter=run.max_iter, tol=run.tol)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("run,mode", PARAMS, ids=[f"{r.id}-{m}" for r, m in PARAMS])
def test_solve_within_K_of_reference(run, mode):
    """Checks (a)-(h) of one run in one mode; prints every ratio."""
    dc, dp, info = _solve(run, mode)
    m = C.check(run, dc, dp, info, mode, oracle_iters=int(C.oracle(run)[2][0]))
    again = _solve(run, mode)
    for a, b, what in zip((dc, dp, info), again, ("dc", "dp", "info")):
        np.testing.assert_array_equal(a, b, err_msg=f"{run.id} {mode}: second call, {what}")
    for u in C.UNITS:
        if u in m:
            _worst[u, mode] = max(_worst.get((u, mode), 0.0), m[u])
            _worst[u, run.name] = max(_worst.get((u, run.name), 0.0), m[u])


def test_fallback_preconditioner_after_one_iteration():
    """After one iteration dc = x_1 = α M b: the fallback camera's dc is its diagonal
    preconditioner's, the other cameras' their block inverse's, per camera within K_FIRST units
    of the 50-digit x_1 (ba_solve_cases.first_ratio)."""
    for run in C.FIRST_RUNS:
        for mode in C.MODES:
            if (run, mode) not in PARAMS:
                continue
            dc, _, info = _solve(run, mode)
            r, _ = C.first_ratio(run, dc)
            print(f"first iterate {run.id} {mode}: {r:.3g} units (K = {C.K_FIRST:.3g})")
            assert info[4] == C.FLAG_FALLBACK and info[0] == 1 and r <= C.K_FIRST, (run.id, mode)


def test_worst_ratios_summary():
    """Prints the worst ratio per unit and mode, and per unit and case, of this process's solves."""
    for u in C.UNITS:
        by_mode = " ".join(f"{m}={_worst[u, m]:.3g}" for m in C.MODES if (u, m) in _worst)
        names = dict.fromkeys(r.name for r in C.RUNS)
        by_case = " ".join(f"{n}={_worst[u, n]:.3g}" for n in names if (u, n) in _worst)
        print(f"kernel worst {u} (K = {C.K[u]:.3g}): {by_mode} | {by_case}")
