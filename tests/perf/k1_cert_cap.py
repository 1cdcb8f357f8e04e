"""What the mutual certificate's threat walk costs against the reverse scan it replaces: the
measurement behind CERT_CAP_DEFAULT (csrc/match_l2fr.hip).  The bench scene with ratio 65535/1
makes every query a survivor and nearly every query a threat, so a cap nothing exceeds walks
threats x survivors units per pair; the same call with SFM_L2FR_CERT=0 pays the reverse scan.
Prints the whole-GPU time per unit and per exact dot product and, from the reverse scan's
whole-GPU time per pair at this K, the break-even units per pair.
python tests/perf/k1_cert_cap.py  (N_IMG, K, ROUNDS override; default 16 x 2048, all pairs)"""
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
    n_img, k = int(os.environ.get("N_IMG", "16")), int(os.environ.get("K", "2048"))
    rounds = int(os.environ.get("ROUNDS", "3"))
    s = synth.make_scene(n_img, k, seed=0)
    pairs = synth.unordered_pairs(n_img)
    ctx = sfmcore.context(0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    desc, n_kp, pr = T(s["desc"]), T(s["n_kp"]), T(pairs)
    legs = {"ratio_only": dict(xc=sfmcore.XC_NONE, env={"SFM_L2_PATH": "fr"}),
            "reverse_scan": dict(xc=sfmcore.XC_MUTUAL, env={"SFM_L2_PATH": "fr", "SFM_L2FR_CERT": "0"}),
            "certificate": dict(xc=sfmcore.XC_MUTUAL, env={"SFM_L2_PATH": "fr",
                                                           "SFM_L2FR_CERT_CAP": str(1 << 40)})}
    ms = {l: [] for l in legs}
    out = {}
    for _ in range(rounds + 1):   # the first round untimed
        for leg, cfg in legs.items():
            os.environ.update(cfg["env"])
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            out[leg] = ctx.match_batch(desc, n_kp, pr, cross_check=cfg["xc"], ratio=(65535, 1))
            ev[1].record()
            torch.cuda.synchronize()
            ms[leg].append(ev[0].elapsed_time(ev[1]))
            for kk in cfg["env"]:
                os.environ.pop(kk, None)
    ms = {l: t[1:] for l, t in ms.items()}
    os.environ.update(legs["certificate"]["env"])
    ctx.match_cert_stats(enable=True)
    ctx.match_batch(desc, n_kp, pr, cross_check=sfmcore.XC_MUTUAL, ratio=(65535, 1))
    certified, flagged, dots = ctx.match_cert_stats(enable=False, read=True)
    for kk in legs["certificate"]["env"]:
        os.environ.pop(kk, None)
    same = bool((out["reverse_scan"][0] == out["certificate"][0]).all())
    nk = s["n_kp"].astype(np.float64)
    units = float(np.sum(nk[pairs[:, 0]] ** 2))   # threats x survivors <= n_a^2 per pair
    base = min(ms["ratio_only"])
    walk_ms = min(ms["certificate"]) - base
    rev_ms = min(ms["reverse_scan"]) - base
    res = {"n_img": n_img, "k": k, "pairs": int(len(pairs)), "ms": ms, "counts_equal": same,
           "certified": certified, "flagged": flagged, "exact_dots": dots,
           "units_upper_bound": units, "walk_ms": walk_ms, "reverse_scan_and_final_ms": rev_ms,
           "ns_per_exact_dot": walk_ms * 1e6 / max(dots, 1),
           "reverse_us_per_pair": rev_ms * 1e3 / len(pairs),
           "break_even_dots_per_pair": rev_ms / walk_ms * dots / len(pairs) if walk_ms > 0 else None}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
