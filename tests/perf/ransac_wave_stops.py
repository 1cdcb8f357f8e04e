"""Where K2's score waves stop, per hypothesis block (profiles/k2_pilot): one
cfg4-shaped batch (K = 4096, H = 4096, N_PAIRS pairs, default 2048 = 256 per XCD, so the groups
of 64 of xcd_pair_block are in effect) is scored with sfm_ransac_stats on, and
sfm_ransac_wave_stops gives every wave's matches scored past the preview.  Prints the mean of
stop / (M - PV) per hypothesis block hb = 0..H/256-1 (rank order: block 0 holds the best
previews), per wave of block 0, and the batch's executed share.  A block that starts without a
bound shows a share near 1; one that starts with the final bound shows the later blocks' share.
Usage: python tests/perf/ransac_wave_stops.py [out.json]   (SFM_RANSAC_PILOT / _GROUP apply)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "sfm-project_amd")]

import numpy as np
import torch

import sfmcore
import synth

PV = 128


def main():
    n_pairs = int(os.environ.get("N_PAIRS", "2048"))
    H = int(os.environ.get("N_HYP", "4096"))
    n_img = 2
    while n_img * (n_img - 1) // 2 < n_pairs:
        n_img += 1
    s = synth.make_scene(n_img, 4096, seed=0)
    pairs = synth.unordered_pairs(n_img)[:n_pairs]
    ctx = sfmcore.context(0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    desc, n_kp, kps, pr = T(s["desc"]), T(s["n_kp"]), T(s["kps"]), T(pairs)
    cnt, mt, _ = ctx.match_batch(desc, n_kp, pr, ratio=(4, 5))
    ctx.ransac_batch(kps, pr, cnt, mt, n_hyp=H)      # warm-up, not counted
    ctx.ransac_stats(enable=True, read=True)          # reset
    out = ctx.ransac_batch(kps, pr, cnt, mt, n_hyp=H)
    stops = ctx.ransac_wave_stops(n_pairs, H).astype(np.float64)
    ex, al, npairs = ctx.ransac_stats(enable=False, read=True)
    M = cnt.cpu().numpy().astype(np.int64)
    ic = out["inl_count"].cpu().numpy()
    sel = M > PV + 64
    share = stops[sel] / (M[sel] - PV)[:, None]       # [pairs, H/64]
    per_hb = share.reshape(sel.sum(), H // 256, 4).mean(axis=(0, 2))
    per_w0 = share[:, :4].mean(axis=0)
    res = {"pairs": int(n_pairs), "pairs_in_table": int(sel.sum()), "n_hyp": H,
           "pilot": os.environ.get("SFM_RANSAC_PILOT", "default"),
           "mean_M": float(M.mean()), "mean_best": float(ic[M >= 8].mean()),
           "executed_frac": ex / al, "score_share": float(share.mean()),
           "share_per_hb": [round(float(x), 4) for x in per_hb],
           "share_per_wave_of_block0": [round(float(x), 4) for x in per_w0]}
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
