"""Image retrieval for pair selection on bench.local_scene(500, 4096), one
process, one JSON line per part:
  stages      per vocabulary size: seconds of select_pairs' stages (median of REPS runs after a
              warm-up); the assign kernel's i8 rate as a fraction of the nominal dense-i8 peak and
              of the MFMA-only calibration loop (sfm_calib_mfma_i8) measured in the same run
  sweep       n_words in N_WORDS x k in {16, 24, 32, 48}: selected pairs and the recall against
              the pairs the all-pairs run verifies on the same device (all verified pairs, those
              with >= 60 inliers, and weighted by verified rows)
  end_to_end  incremental.reconstruct with all pairs against pairs="retrieval" (the defaults, and
              each --e2e "n_words:k" setting), interleaved, median of RUNS runs each: match_verify
              and total seconds, registered images, points, median reprojection error
Usage: python tests/perf/retrieval_time.py [--n-img 500] [--k 4096] [--reps 7] [--runs 5]
                                           [--n-words 4096,16384,65536] [--e2e 4096:32]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "sfm-project_amd"), ROOT]

import numpy as np
import torch

import bench
import incremental
import match_graph
import reconstruction as R
import retrieval
import sfmcore

KS = (16, 24, 32, 48)


def median_reprojection(rec, scene):
    tptr, timg, tkp = rec.tracks
    obs_track = np.repeat(np.arange(len(tptr) - 1), np.diff(tptr))
    use = rec.has_point[obs_track] & rec.registered[timg]
    pts_ids, pt_idx = np.unique(obs_track[use], return_inverse=True)
    err = R.reprojection_errors(rec.cams, scene["pp"], rec.points[pts_ids], timg[use],
                                pt_idx.astype(np.int32), scene["kps"][timg[use], tkp[use]])
    return float(np.median(err))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-img", type=int, default=500)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--n-words", default="4096,16384,65536")
    ap.add_argument("--e2e", default="4096:32", help="extra end-to-end settings n_words:k,...")
    a = ap.parse_args()
    n_words_list = [int(x) for x in a.n_words.split(",")]
    scene, grid = bench.local_scene(a.n_img, a.k)
    desc, kps, n_kp = scene["desc"], scene["kps"], scene["n_kp"]
    intr = np.c_[scene["cams"][:, 6:8], scene["pp"]]
    ctx = sfmcore.context(0)
    desc_t = torch.from_numpy(desc).cuda()
    n_kp_t = torch.from_numpy(n_kp).cuda()
    n_pairs_all = a.n_img * (a.n_img - 1) // 2
    total = int(n_kp.sum())

    # ---- stage times
    calib = {k: float(v) for k, v in ctx.calib_mfma_i8().items()}
    for nw in n_words_list:
        nw = min(nw, total)
        retrieval.select_pairs(desc_t, n_kp_t, n_words=nw)
        runs = [retrieval.select_pairs(desc_t, n_kp_t, n_words=nw, return_info=True)[1]["timings"]
                for _ in range(a.reps)]
        stages = {s: float(np.median([r[s] for r in runs])) for s in runs[0]}
        # the kernel scores every row of the padded [n_img * k_max] array against n_words padded
        # to 128; on this scene every row is valid, so executed = useful up to the word padding
        ops = 2.0 * total * nw * 128
        tops = ops / stages["assign"] / 1e12
        print(json.dumps({"part": "stages", "scene": f"local_scene({a.n_img}, {a.k})",
                          "grid": list(grid), "n_words": nw, "reps": a.reps, "seconds": stages,
                          "total_s": float(sum(stages.values())), "assign_tops": tops,
                          "assign_frac_dense_i8": tops / bench.PEAK_I8_TOPS,
                          "calib_mfma_i8": calib, "assign_frac_calib": tops / calib["tops"]}),
              flush=True)

    # ---- the all-pairs run's verified pairs on this device
    pairs = np.stack(np.triu_indices(a.n_img, 1), axis=1).astype(np.int32)
    gb = match_graph.GraphBuilder(desc, kps, n_kp, device=0)
    pairs_t = torch.from_numpy(pairs).cuda()
    rows, inl = incremental._match_graph(gb, pairs, pairs_t, n_kp, None)
    rows_per_pair = torch.bincount(rows[:, 0].long(), minlength=len(pairs)).cpu().numpy()
    verified = rows_per_pair > 0
    strong = verified & (inl >= 60)
    del gb, rows
    key_all = pairs[:, 0].astype(np.int64) * a.n_img + pairs[:, 1]
    for nw in n_words_list:
        for k in KS:
            sel = retrieval.select_pairs(desc_t, n_kp_t, k=k, n_words=nw)
            hit = np.isin(key_all, sel[:, 0].astype(np.int64) * a.n_img + sel[:, 1])
            print(json.dumps({
                "part": "sweep", "n_words": nw, "k": k, "selected_pairs": int(len(sel)),
                "all_pairs": n_pairs_all, "selected_frac": len(sel) / n_pairs_all,
                "verified_pairs": int(verified.sum()),
                "recall_verified": float((hit & verified).sum() / max(verified.sum(), 1)),
                "strong_pairs": int(strong.sum()),
                "recall_ge60": float((hit & strong).sum() / max(strong.sum(), 1)),
                "recall_rows": float(rows_per_pair[hit].sum() / max(rows_per_pair.sum(), 1))}),
                  flush=True)

    # ---- end to end, interleaved
    legs = [("all", {}), ("retrieval_default", dict(pairs="retrieval"))]
    for spec in filter(None, a.e2e.split(",")):
        nw, k = (int(x) for x in spec.split(":"))
        legs.append((f"retrieval_{nw}_{k}", dict(pairs="retrieval",
                                                 retrieval=dict(n_words=nw, k=k))))
    out = {name: [] for name, _ in legs}
    for r in range(a.runs + 1):
        for name, kw in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = incremental.reconstruct(desc, kps, n_kp, intr, **kw)
            torch.cuda.synchronize()
            tot = time.perf_counter() - t0
            if r == 0:
                continue                      # warm-up of every leg
            out[name].append(dict(total_s=tot, match_verify_s=rec.timings["match_verify"],
                                  select_pairs_s=rec.timings.get("select_pairs", 0.0),
                                  registered=int(rec.registered.sum()),
                                  points=int(rec.has_point.sum()), n_verified=rec.n_verified,
                                  pairs=int(len(rec.pairs)),
                                  median_reproj_px=median_reprojection(rec, scene)))
    res = {"part": "end_to_end", "runs": a.runs}
    for name, rs in out.items():
        res[name] = {k: float(np.median([x[k] for x in rs])) for k in rs[0]}
        res[name]["total_s_all_runs"] = [x["total_s"] for x in rs]
        res[name]["speedup_total"] = res["all"]["total_s"] / res[name]["total_s"]
        res[name]["speedup_match_verify"] = res["all"]["match_verify_s"] / (
            res[name]["match_verify_s"] + res[name]["select_pairs_s"])
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
