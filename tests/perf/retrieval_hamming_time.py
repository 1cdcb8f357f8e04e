"""Retrieval on binary descriptors (DESIGN.md §4.11 "Hamming"), one process on one device; writes
<out>/retrieval_hamming_time.jsonl (one JSON line per part) and <out>/README.md (the same figures
as tables):
  assign     ctx.vocab_assign at n_img x k descriptors against each vocabulary size, the Hamming
             kernel (32-byte rows of the ORB grid scene) and the L2 kernel (128-byte random rows;
             its time does not depend on the data), alternating, device events around each call,
             median of REPS after WARM warm-up calls.  The L2 call includes its vocabulary prep
             kernel.  Ratio Hamming / L2 (the Hamming kernel does twice the MFMA work) and each
             call's i8 rate as a fraction of the nominal dense-i8 peak and of the MFMA-only
             calibration loop (sfm_calib_mfma_i8) of the same run.
  majority   one ctx.vocab_majority round on the words of that assignment, the same way
  stages     retrieval.select_pairs end to end, stage by stage (host clock, each stage ends in a
             device synchronise), with every default and with n_words=4096, lloyd=2
Usage: python tests/perf/retrieval_hamming_time.py [--n-img 500] [--k 4096] [--reps 9]
           [--n-words 4096,16384,65536] [--out profiles/retrieval_hamming]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "sfm-project_amd"), ROOT]

import numpy as np
import torch

import bench
import retrieval
import sfmcore

WARM = 3


def orb_grid_scene(n_img, k):
    """bench.local_scene's recipe (the cfg5 view grid) with ORB-like descriptors."""
    import synth
    n_el = max(1, int(round((n_img / 2) ** 0.5)))
    grid = (-(-n_img // n_el), n_el, bench.CFG5_GRID[2], bench.CFG5_GRID[3])
    return synth.make_scene(n_img, k, seed=bench.CFG5_SEED, k1_range=0.02, window=bench.CFG5_WINDOW,
                            grid=grid, track_len=bench.CFG5_TRACK, orb=True), grid


def timed(fns, reps):
    """Median milliseconds of each callable, alternating them: WARM untimed rounds, then `reps`
    rounds with device events around every call."""
    ms = [[] for _ in fns]
    for r in range(WARM + reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= WARM:
                ms[i].append(e0.elapsed_time(e1))
    return [float(np.median(m)) for m in ms], [[float(min(m)), float(max(m))] for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-img", type=int, default=500)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--n-words", default="4096,16384,65536")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_hamming"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    scene, grid = orb_grid_scene(a.n_img, a.k)
    ctx = sfmcore.context(0)
    desc_h = torch.from_numpy(scene["desc"]).cuda()
    n_kp = torch.from_numpy(scene["n_kp"]).cuda()
    total = int(scene["n_kp"].sum())
    gen = torch.Generator(device="cuda").manual_seed(1)
    desc_l = torch.randint(0, 256, desc_h.shape[:2] + (128,), dtype=torch.uint8, device="cuda",
                           generator=gen)
    calib = {k: float(v) for k, v in ctx.calib_mfma_i8().items()}
    shape = f"{a.n_img} x {a.k}"

    for nw in (int(x) for x in a.n_words.split(",")):
        nw = min(nw, total)
        voc_h = retrieval.sample_vocabulary(desc_h, n_kp, nw, 0)
        voc_l = retrieval.sample_vocabulary(desc_l, n_kp, nw, 0)
        out = (torch.empty(desc_h.shape[:2], dtype=torch.int32, device="cuda"), None)
        (t_h, t_l), (r_h, r_l) = timed(
            [lambda: ctx.vocab_assign(desc_h, n_kp, voc_h, with_dist=False, out=out),
             lambda: ctx.vocab_assign(desc_l, n_kp, voc_l, with_dist=False, out=out)], a.reps)
        # executed MFMA work: every row of the padded array against n_words padded to 128
        ops_l = 2.0 * a.n_img * a.k * (-(-nw // 128) * 128) * 128
        ops_h = 2.0 * ops_l
        tops_h, tops_l = ops_h / t_h / 1e9, ops_l / t_l / 1e9
        emit({"part": "assign", "descriptors": shape, "n_words": nw, "reps": a.reps,
              "hamming_ms": t_h, "hamming_ms_min_max": r_h, "l2_ms": t_l, "l2_ms_min_max": r_l,
              "ratio_hamming_over_l2": t_h / t_l, "hamming_tops": tops_h, "l2_tops": tops_l,
              "hamming_frac_dense_i8": tops_h / bench.PEAK_I8_TOPS,
              "l2_frac_dense_i8": tops_l / bench.PEAK_I8_TOPS,
              "hamming_frac_calib": tops_h / calib["tops"], "l2_frac_calib": tops_l / calib["tops"],
              "calib_mfma_i8": calib})
        word, _ = ctx.vocab_assign(desc_h, n_kp, voc_h, with_dist=False)
        new = torch.empty_like(voc_h)
        (t_m,), (r_m,) = timed([lambda: ctx.vocab_majority(desc_h, n_kp, word, voc_h, out=new)],
                               a.reps)
        emit({"part": "majority", "descriptors": shape, "n_words": nw, "reps": a.reps,
              "ms": t_m, "ms_min_max": r_m, "counter_bytes": nw * 257 * 4})

    for tag, kw in (("defaults", {}), ("n_words=4096, lloyd=2", dict(n_words=4096, lloyd=2))):
        retrieval.select_pairs(desc_h, n_kp, **kw)
        runs = [retrieval.select_pairs(desc_h, n_kp, return_info=True, **kw)
                for _ in range(a.reps)]
        stages = {s: float(np.median([r[1]["timings"][s] for r in runs]))
                  for s in runs[0][1]["timings"]}
        emit({"part": "stages", "scene": f"ORB grid scene {shape}", "grid": list(grid),
              "setting": tag, "n_words": int(runs[0][1]["vocab"].shape[0]), "reps": a.reps,
              "seconds": stages, "total_s": float(sum(stages.values())),
              "selected_pairs": int(len(runs[0][0])),
              "all_pairs": a.n_img * (a.n_img - 1) // 2})

    with open(os.path.join(a.out, "retrieval_hamming_time.jsonl"), "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(readme(lines, shape, calib))


def readme(lines, shape, calib):
    o = ["# Retrieval on binary descriptors: measured times", "",
         "Written by `tests/perf/retrieval_hamming_time.py` from one run in one process on one "
         "MI355X; the raw records are in `retrieval_hamming_time.jsonl`.  Medians of "
         f"{lines[0]['reps']} calls after {WARM} warm-up calls, device events around each call, the "
         "two assign kernels alternating.  The calibration loop (MFMA only, register operands) "
         f"reached {calib['tops']:.0f} TOP/s i8 in this run; the nominal dense-i8 peak is "
         f"{bench.PEAK_I8_TOPS:.0f} TOP/s.", "",
         f"## Assign, {shape} descriptors", "",
         "The Hamming kernel does twice the MFMA work of the L2 kernel at equal shapes (256 against "
         "128 expanded bytes per row).  The L2 call includes its vocabulary prep kernel.", "",
         "| words | Hamming ms | L2 ms | ratio | Hamming: of dense i8 / of calibration | "
         "L2: of dense i8 / of calibration |", "|---|---|---|---|---|---|"]
    for r in (x for x in lines if x["part"] == "assign"):
        o.append(f"| {r['n_words']} | {r['hamming_ms']:.2f} | {r['l2_ms']:.2f} | "
                 f"{r['ratio_hamming_over_l2']:.2f} | {r['hamming_frac_dense_i8']:.3f} / "
                 f"{r['hamming_frac_calib']:.3f} | {r['l2_frac_dense_i8']:.3f} / "
                 f"{r['l2_frac_calib']:.3f} |")
    o += ["", "## One k-majority round", "", "| words | ms | counters |", "|---|---|---|"]
    for r in (x for x in lines if x["part"] == "majority"):
        o.append(f"| {r['n_words']} | {r['ms']:.2f} | {r['counter_bytes'] / 2**20:.1f} MiB |")
    o += ["", f"## select_pairs on the ORB grid scene, {shape}", "",
          "Seconds per stage (host clock, every stage ends in a device synchronise).", ""]
    st = [x for x in lines if x["part"] == "stages"]
    keys = list(st[0]["seconds"])
    o += ["| setting | words | " + " | ".join(keys) + " | total | pairs selected |",
          "|---|---|" + "---|" * (len(keys) + 2)]
    for r in st:
        o.append(f"| {r['setting']} | {r['n_words']} | "
                 + " | ".join(f"{r['seconds'][k]:.4f}" for k in keys)
                 + f" | {r['total_s']:.4f} | {r['selected_pairs']} of {r['all_pairs']} |")
    return "\n".join(o) + "\n"


if __name__ == "__main__":
    main()
