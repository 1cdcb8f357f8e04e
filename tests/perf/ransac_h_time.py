"""Homography RANSAC against the F RANSAC on cfg3's tentative matches:
synth.make_scene(50, 2048), the 1225 unordered pairs, match_batch with ratio 4/5, 4096 hypotheses.
ransac_batch (thr 1.0) and ransac_h_batch (thr 4.0) are timed alternately in one process with
device events after a warm-up; prints one JSON line with both medians and their ratio.  The
yardstick is the F batch of the same run, not an absolute time.  SFMCORE_LIB selects a
variant build (tools/build_variant.sh, e.g. -DRANSAC_H_ABL_NOPRUNE: the H batch without pruning).
Usage: python tests/perf/ransac_h_time.py   (REPS repetitions each, default 30)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "sfm-project_amd")]

import numpy as np
import torch

import sfmcore
import synth


def main():
    reps = max(int(os.environ.get("REPS", "30")), 20)
    n_hyp = 4096
    s = synth.make_scene(50, 2048, seed=0)
    pairs = synth.unordered_pairs(50)
    ctx = sfmcore.context(0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    desc, n_kp, kps, pr = T(s["desc"]), T(s["n_kp"]), T(s["kps"]), T(pairs)
    cnt, mt, _ = ctx.match_batch(desc, n_kp, pr, ratio=(4, 5))
    of = ctx.ransac_batch(kps, pr, cnt, mt, n_hyp=n_hyp, thr=1.0)
    oh = ctx.ransac_h_batch(kps, pr, cnt, mt, n_hyp=n_hyp, thr=4.0)
    run_f = lambda: ctx.ransac_batch(kps, pr, cnt, mt, n_hyp=n_hyp, thr=1.0, out=of)
    run_h = lambda: ctx.ransac_h_batch(kps, pr, cnt, mt, n_hyp=n_hyp, thr=4.0, out=oh)
    for _ in range(5):
        run_f()
        run_h()
    torch.cuda.synchronize()
    times = {"f": [], "h": []}
    for _ in range(reps):
        for name, fn in (("f", run_f), ("h", run_h)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    f_ms, h_ms = float(np.median(times["f"])), float(np.median(times["h"]))
    M = cnt.cpu().numpy()
    fc, hc = of["inl_count"].cpu().numpy(), oh["inl_count"].cpu().numpy()
    print(json.dumps(dict(
        scene="cfg3 make_scene(50, 2048)", pairs=int(len(pairs)), n_hyp=n_hyp, reps=reps,
        mean_matches=round(float(M.mean()), 1), mean_f_inliers=round(float(fc.mean()), 1),
        mean_h_inliers=round(float(hc.mean()), 1),
        lib=os.path.basename(sfmcore.LIB_PATH),
        f_ms=round(f_ms, 4), h_ms=round(h_ms, 4),
        f_ms_min=round(float(np.min(times["f"])), 4), h_ms_min=round(float(np.min(times["h"])), 4),
        h_over_f=round(h_ms / f_ms, 4))), flush=True)


if __name__ == "__main__":
    main()
