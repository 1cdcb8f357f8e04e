"""Guided matching, timed on one GPU in one process, one JSON line per part:
  cfg3        synth.make_scene(50, 2048, seed=0), all 1225 pairs: event time of K1 (match_batch),
              K2 (ransac_batch), the guided call and the second K2, interleaved, median of REPS
              rounds after a warm-up; per verified pair; inliers before and after
  local       the cfg5 local-visibility scene (bench.local_scene) at --local-n-img x --local-k, all
              pairs, where a few per cent verify: the same, plus the guided call's time per pair
              of the batch (what the early exit of the unverified pairs costs)
  end_to_end  incremental.reconstruct on bench.local_scene(--n-img, --k), guided=None against
              guided=True, interleaved, median of RUNS runs after a warm-up of both
Usage: python tests/perf/guided_time.py [--reps 7] [--runs 3] [--local-n-img 200] [--local-k 4096]
                                        [--n-img 500] [--k 4096] [--parts cfg3,local,end_to_end]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "sfm-project_amd"), ROOT]

import numpy as np
import torch

torch.set_num_threads(min(16, torch.get_num_threads()))

import bench
import incremental
import match_graph
import reconstruction as R
import synth


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    return out, (e0, e1)


def stage_times(scene, pairs, reps, label):
    gb = match_graph.GraphBuilder(scene["desc"], scene["kps"], scene["n_kp"], guided=True)
    pairs_t = torch.from_numpy(np.ascontiguousarray(pairs)).cuda()
    P = len(pairs)
    b = gb._buffers(P)
    ev = {k: [] for k in ("k1", "k2", "guided", "k2_guided")}
    for r in range(reps + 1):
        (count, match, _), e_k1 = timed(lambda: gb.match(pairs_t))
        rs, e_k2 = timed(lambda: gb.verify(pairs_t, count, match))
        (gc, gm, _), e_g = timed(lambda: gb.guided_match(pairs_t, rs))
        rs2, e_k2g = timed(lambda: gb.ctx.ransac_batch(gb.kps, pairs_t, gc, gm,
                                                       out=b["guided_ransac"], **gb.ransac_kw))
        torch.cuda.synchronize()
        if r == 0:
            continue                                  # warm-up round
        for k, (a, z) in zip(ev, (e_k1, e_k2, e_g, e_k2g)):
            ev[k].append(a.elapsed_time(z))
    ms = {k: float(np.median(v)) for k, v in ev.items()}
    inl1, inl2 = rs["inl_count"].cpu().numpy(), rs2["inl_count"].cpu().numpy()
    ver1, ver2 = inl1 >= gb.min_inliers, inl2 >= gb.min_inliers
    nv = max(int(ver1.sum()), 1)
    print(json.dumps({
        "part": label, "pairs": P, "k_max": int(gb.k_max), "reps": reps, "median_ms": ms,
        "all_rounds_ms": ev, "verified_pairs_first": int(ver1.sum()),
        "verified_pairs_second": int(ver2.sum()),
        "inliers_first": int(inl1[ver1].sum()), "inliers_second": int(inl2[ver2].sum()),
        "tentative_first": int(count.sum().item()), "tentative_guided": int(gc.sum().item()),
        "us_per_verified_pair": {k: 1e3 * v / nv for k, v in ms.items()},
        "guided_us_per_batch_pair": 1e3 * ms["guided"] / P}), flush=True)


def median_reprojection(rec, scene):
    tptr, timg, tkp = rec.tracks
    obs_track = np.repeat(np.arange(len(tptr) - 1), np.diff(tptr))
    use = rec.has_point[obs_track] & rec.registered[timg]
    pts_ids, pt_idx = np.unique(obs_track[use], return_inverse=True)
    err = R.reprojection_errors(rec.cams, scene["pp"], rec.points[pts_ids], timg[use],
                                pt_idx.astype(np.int32), scene["kps"][timg[use], tkp[use]])
    return float(np.median(err))


def end_to_end(n_img, k, runs):
    scene, _ = bench.local_scene(n_img, k)
    intr = np.c_[scene["cams"][:, 6:8], scene["pp"]]
    legs = [("default", None), ("guided", True)]
    out = {name: [] for name, _ in legs}
    for r in range(runs + 1):
        for name, g in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = incremental.reconstruct(scene["desc"], scene["kps"], scene["n_kp"], intr,
                                          guided=g)
            torch.cuda.synchronize()
            tot = time.perf_counter() - t0
            if r == 0:
                continue
            out[name].append(dict(total_s=tot, match_verify_s=rec.timings["match_verify"],
                                  registered=int(rec.registered.sum()),
                                  points=int(rec.has_point.sum()), n_verified=rec.n_verified,
                                  median_reproj_px=median_reprojection(rec, scene)))
    res = {"part": "end_to_end", "scene": f"bench.local_scene({n_img}, {k})", "runs": runs}
    for name, rs in out.items():
        res[name] = {key: float(np.median([x[key] for x in rs])) for key in rs[0]}
        res[name]["total_s_all_runs"] = [x["total_s"] for x in rs]
    res["added_total_s"] = res["guided"]["total_s"] - res["default"]["total_s"]
    res["added_match_verify_s"] = (res["guided"]["match_verify_s"]
                                   - res["default"]["match_verify_s"])
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--local-n-img", type=int, default=200)
    ap.add_argument("--local-k", type=int, default=4096)
    ap.add_argument("--n-img", type=int, default=500)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--parts", default="cfg3,local,end_to_end")
    a = ap.parse_args()
    parts = a.parts.split(",")
    if "cfg3" in parts:
        stage_times(synth.make_scene(50, 2048, seed=0), synth.unordered_pairs(50), a.reps, "cfg3")
    if "local" in parts:
        scene, _ = bench.local_scene(a.local_n_img, a.local_k)
        stage_times(scene, synth.unordered_pairs(a.local_n_img), a.reps, "local")
    if "end_to_end" in parts:
        end_to_end(a.n_img, a.k, a.runs)


if __name__ == "__main__":
    main()
