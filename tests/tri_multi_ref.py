"""CPU statement of sfm_triangulate_multi (TEST INFRASTRUCTURE ONLY): a numpy loop that calls
tri_ref.run, the CPU statement of sfm_triangulate_robust, once per round on the compacted
remainder with seed + r, and applies the acceptance rule of include/sfmcore.h."""
from __future__ import annotations

import numpy as np

import tri_ref


def run(tab, pt_ptr, cam_idx, uv, pt_id, max_points=3, min_views=2, thr=4.0, min_angle_deg=1.0,
        max_hyp=64, seed=42):
    """(pts [n,R,3], stats [n,R,4], info [n,R,2] i32, n_points [n] i32, label [n_obs] i8) as
    Context.triangulate_multi returns them."""
    pt_ptr = np.ascontiguousarray(pt_ptr, np.int32)
    cam_idx = np.ascontiguousarray(cam_idx, np.int32)
    uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
    pt_id = np.ascontiguousarray(pt_id, np.int32)
    n, R = len(pt_ptr) - 1, int(max_points)
    pts, stats = np.zeros((n, R, 3)), np.zeros((n, R, 4))
    stats[:, :, 3] = 5.0
    info = np.zeros((n, R, 2), np.int32)
    info[:, :, 1] = -1
    n_points = np.zeros(n, np.int32)
    label = np.full(len(cam_idx), -1, np.int8)
    # the running sub-problem: tracks `trk` with the observations `obs` (indices into the input)
    trk = np.arange(n)
    obs = [np.arange(pt_ptr[t], pt_ptr[t + 1]) for t in range(n)]
    for r in range(R):
        if len(trk) == 0:
            break
        ptr = np.r_[0, np.cumsum([len(o) for o in obs])].astype(np.int32)
        o_all = np.concatenate(obs).astype(np.int64) if ptr[-1] else np.zeros(0, np.int64)
        rp, rs, rm, ri = tri_ref.run(tab, ptr, cam_idx[o_all], uv[o_all], pt_id[trk], thr=thr,
                                     min_angle_deg=min_angle_deg, max_hyp=max_hyp,
                                     seed=(int(seed) + r) & 0xFFFFFFFFFFFFFFFF)
        nxt_trk, nxt_obs = [], []
        for s, t in enumerate(trk):
            status = int(rs[s, 3])
            ok = status == 0 and (r == 0 or ri[s, 0] >= min_views)
            if r == 0 or ok:
                pts[t, r], stats[t, r], info[t, r] = rp[s], rs[s], ri[s]
            else:
                stats[t, r, 3] = status if status != 0 else 5
            if not ok:
                continue
            n_points[t] = r + 1
            m = rm[ptr[s]:ptr[s + 1]].astype(bool)
            label[obs[s][m]] = r
            if r + 1 < R:
                nxt_trk.append(t)
                nxt_obs.append(obs[s][~m])
        trk, obs = np.array(nxt_trk, np.int64), nxt_obs
    return pts, stats, info, n_points, label


def host_loop(tab, prob, **kw):
    """run() on a problem dict of tri_cases / tri_multi_cases."""
    return run(tab, prob["pt_ptr"], prob["cam_idx"], prob["uv"], prob["pt_id"], **kw)
