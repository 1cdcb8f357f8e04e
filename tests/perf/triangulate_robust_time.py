"""sfm_triangulate_robust against sfm_triangulate, device-event timed in one
process after a warm-up, the two calls alternating:
  cfg5 shape  100 k tracks x 5 views   (synth.make_ba_problem, 0.5 px noise)
  arc shape   4 k tracks x 200 views
  mixed       20 k tracks of 2 .. 300 views (every bin of the robust kernel)
Per problem: microseconds of both calls (median and minimum), and the robust call's time on each
hypothesis-count bin's tracks alone (the kernel launches one grid per bin; a bin's share is its
time over the sum).  One JSON line per problem.
Usage: python tests/perf/triangulate_robust_time.py   (REPS repetitions each, default 30)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "sfm-project_amd")]

import numpy as np
import torch

import sfmcore
import synth

BINS = ((0, 8), (8, 16), (16, 32), (32, 1 << 30))     # hypothesis counts (lo, hi]
SHORT_MAX_OBS = 16                                    # longer tracks: the last bin (tri_bin)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)) * 1e3, float(np.min(ms)) * 1e3


def subset(ptr, cam_idx, uv, tracks):
    n = np.diff(ptr)[tracks]
    obs = np.concatenate([np.arange(ptr[t], ptr[t + 1]) for t in tracks]) if len(tracks) else \
        np.zeros(0, np.int64)
    return np.r_[0, np.cumsum(n)].astype(np.int32), cam_idx[obs], uv[obs]


def measure(name, n_cam, n_pt, obs_per_pt, reps, max_hyp=64):
    prob = synth.make_ba_problem(n_cam, n_pt, obs_per_pt=obs_per_pt, seed=0, noise_px=0.5,
                                 perturb=0.0)
    ptr = np.r_[0, np.cumsum(np.bincount(prob["pt_idx"], minlength=n_pt))].astype(np.int32)
    ctx = sfmcore.context(0)
    T = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    cams, pp = T(prob["cams"], np.float64), T(prob["pp"], np.float64)

    def calls(p, ci, uv, ids):
        p, ci, uv, ids = T(p, np.int32), T(ci, np.int32), T(uv, np.float64), T(ids, np.int32)
        return (lambda: ctx.triangulate(cams, pp, p, ci, uv),
                lambda: ctx.triangulate_robust(cams, pp, p, ci, uv, ids, max_hyp=max_hyp))

    dlt, rob = calls(ptr, prob["cam_idx"], prob["uv"], np.arange(n_pt))
    pts, st, mask, info = rob()
    st, info = st.cpu().numpy(), info.cpu().numpy()
    d_med, d_min = timed(dlt, reps)
    r_med, r_min = timed(rob, reps)
    n = np.diff(ptr).astype(np.int64)
    n_hyp = np.minimum(n * (n - 1) // 2, max_hyp)
    bins = {}
    key = np.where(n > SHORT_MAX_OBS, 1 << 30, n_hyp)
    for lo, hi in BINS:
        tr = np.nonzero((n >= 2) & (key > lo) & (key <= hi))[0]
        if len(tr) == 0:
            continue
        _, rb = calls(*subset(ptr, prob["cam_idx"], prob["uv"], tr), tr)
        bins[f"{lo + 1}..{hi if hi < 1 << 30 else ''}"] = dict(
            tracks=int(len(tr)), observations=int(n[tr].sum()), us=round(timed(rb, reps)[0], 1))
    tot = sum(b["us"] for b in bins.values())
    for b in bins.values():
        b["share"] = round(b["us"] / tot, 3)
    print(json.dumps(dict(
        problem=name, tracks=n_pt, observations=int(ptr[-1]), max_hyp=max_hyp, reps=reps,
        device=torch.cuda.get_device_name(0), lib=os.path.basename(sfmcore.LIB_PATH),
        triangulate_us=round(d_med, 1), triangulate_us_min=round(d_min, 1),
        robust_us=round(r_med, 1), robust_us_min=round(r_min, 1),
        ratio=round(r_med / d_med, 2), status_ok=int((st[:, 3] == 0).sum()),
        mean_consensus=round(float(info[:, 0].mean()), 2), bins=bins)), flush=True)


def main():
    reps = max(int(os.environ.get("REPS", "30")), 3)
    measure("cfg5 shape: 100k x 5", 500, 100000, 5, reps)
    measure("arc shape: 4k x 200", 500, 4000, 200, reps)
    rng = np.random.Generator(np.random.PCG64(3))
    mixed = np.clip(np.rint(2 + rng.exponential(6.0, size=20000)), 2, 300).astype(np.int64)
    mixed[::200] = 300
    measure("mixed: 20k x 2..300", 500, 20000, mixed, reps)


if __name__ == "__main__":
    main()
