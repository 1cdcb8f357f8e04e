"""GPU: the BA linearisation (sfm_ba_jtj) and cost (sfm_ba_cost) against the 50-digit reference
on the cases of ba_edge_cases.py, every output within K units, through every form of the call:
plain, chunk mode with 8 and with 3 chunks, and the export form of a shard reduced with
sfm_ba_chunk_tree.  K and the units: ba_edge_cases.py."""
import numpy as np
import pytest

import ba_edge_cases as E
import reconstruction as R
import sfmcore

pytestmark = pytest.mark.gpu

MODES = ("plain", "chunks8", "chunks3", "export8")
_problems, _lin = {}, {}


def _T(a, dt=np.float64):
    import torch
    return torch.from_numpy(np.array(a, dt)).cuda()      # a copy: the cases are read-only


def _problem(ctx, name, mode):
    """(linearise(loss_s), cost(loss_s)) of a case in one mode; device-resident, made once per
    process."""
    if (name, mode) in _problems:
        return _problems[name, mode]
    import torch
    c = E.case(name)
    cams, pts = _T(c["cams"]), _T(c["pts"])
    n_cam, n_pt = len(c["cams"]), len(c["pts"])
    args = (np.array(c["pp"]), np.array(c["cam_idx"]), np.array(c["pt_idx"]), np.array(c["uv"]),
            n_cam, n_pt)
    if mode == "plain":
        pt_ptr, _ = sfmcore.csr_by(c["pt_idx"], n_pt)
        cam_ptr, cam_obs = sfmcore.csr_by(c["cam_idx"], n_cam)
        pp, uv = _T(c["pp"]), _T(c["uv"])
        idx = [_T(c["cam_idx"], np.int32), _T(c["pt_idx"], np.int32)]
        csr = [_T(pt_ptr, np.int32), _T(cam_ptr, np.int32), _T(cam_obs, np.int32)]
        lin = lambda s: ctx.ba_jtj(cams, pp, pts, *idx, uv, *csr, loss_s=s)
        cost = lambda s: ctx.ba_cost(cams, pp, pts, *idx, uv, loss_s=s)
    elif mode == "export8":
        whole = R.BAProblem(*args, chunks=8)
        P = R.BAProblem(*args, chunks=list(whole.chunks.chunk_pt), n_total=8, k0=0)

        def lin(s):
            o = P.linearize(cams, pts, s)
            tot = P.ctx.ba_chunk_tree(torch.cat([o["U"].reshape(8, -1), o["gc"].reshape(8, -1),
                                                 o["cost"].reshape(8, 1)], 1))
            o["U"] = tot[:n_cam * 64].view(n_cam, 8, 8)
            o["gc"] = tot[n_cam * 64:n_cam * 72].view(n_cam, 8)
            o["cost"] = tot[n_cam * 72:]
            return o
        cost = lambda s: P.ctx.ba_chunk_tree(P.cost(cams, pts, s).reshape(8, 1))
    else:
        P = R.BAProblem(*args, chunks=int(mode[-1]))
        lin = lambda s: P.linearize(cams, pts, s)
        cost = lambda s: P.cost(cams, pts, s)
    _problems[name, mode] = (lin, cost)
    return lin, cost


def _host(o):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _linearised(ctx, name, loss_s, mode):
    key = (name, loss_s, mode)
    if key not in _lin:
        _lin[key] = _host(_problem(ctx, name, mode)[0](loss_s))
    return _lin[key]


@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_linearisation_within_K_of_reference(ctx, case):
    """res, W, U, V, gc, gp, cost of every mode within K units of the reference; prints the worst
    ratio per output and mode."""
    name, loss_s = case
    worst = 0.0
    for mode in MODES:
        r = E.check(name, loss_s, _linearised(ctx, name, loss_s, mode), mode)
        worst = max(worst, max(r.values()))
    print(f"{name}@{loss_s:g}: worst ratio over outputs and modes {worst:.3f}")


@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_costs_within_K_and_agree_with_linearisation(ctx, case):
    """sfm_ba_cost (ctx.ba_cost, BAProblem.cost: plain, chunked, export form) against the
    reference cost, and against the cost of the same mode's linearisation within K times the
    summation unit eps sum |rho / 2|: contraction is off, so the three copies of the projection in
    ba.hip give the same rho per observation and only the order of the sums may differ."""
    name, loss_s = case
    ref, unit = E.reference(name, loss_s)
    for mode in MODES:
        got = float(_problem(ctx, name, mode)[1](loss_s).cpu().numpy().reshape(-1)[0])
        lin = float(_linearised(ctx, name, loss_s, mode)["cost"].reshape(-1)[0])
        a = abs(got - ref["cost"]) / unit["cost"]
        b = abs(got - lin) / unit["cost_sum"]
        print(f"{name}@{loss_s:g} {mode}: cost vs reference {a:.3f} units, vs linearisation "
              f"{b:.3f} summation units (allowed {E.K:.2f})")
        assert np.isfinite(got) and a <= E.K and b <= E.K, (mode, got, ref["cost"], lin)


@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_two_calls_bit_identical(ctx, case):
    name, loss_s = case
    for mode in MODES:
        lin, cost = _problem(ctx, name, mode)
        first, again = _linearised(ctx, name, loss_s, mode), _host(lin(loss_s))
        for k in first:
            np.testing.assert_array_equal(first[k], again[k], err_msg=f"{mode} {k}")
        np.testing.assert_array_equal(cost(loss_s).cpu().numpy(), cost(loss_s).cpu().numpy())
