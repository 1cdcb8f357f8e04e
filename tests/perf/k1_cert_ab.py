"""The bench rule (L2 mutual + ratio 4/5) through its implementations, interleaved in one process
on one box, outputs compared bit for bit on every pair:
  parent   the default dispatch of another build of the library (PARENT_LIB=path: the parent
           commit's libsfmcore.so, loaded next to this one; leg skipped when unset)
  mutual   this build, SFM_L2_PATH=mutual (mfma_mutual_kernel, the former default)
  cert     this build, SFM_L2_PATH=fr (the forward-scan path with the mutual certificate: the
           default dispatch for 1536 < k_max <= 4096)
  fr_rev   this build, SFM_L2_PATH=fr SFM_L2FR_CERT=0 (the reverse scan for every pair)
python tests/perf/k1_cert_ab.py  (SHARD=r/n, ROUNDS, WARMUP, REPS, N_IMG, K, LEGS override;
default: the 1/8 cfg4 shard of k1_mutual_ab.py; cfg3: N_IMG=50 K=2048 SHARD=0/1).  `verdict`: the new default is kept
only if its mean is below the baseline's (parent, or mutual without PARENT_LIB) by more than three
times the larger of the two legs' spreads (max - min over the rounds)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "sfm-project_amd")]

import numpy as np
import torch

import match_graph
import sfmcore
import synth

ENV = {"mutual": {"SFM_L2_PATH": "mutual"}, "cert": {"SFM_L2_PATH": "fr"},
       "fr_rev": {"SFM_L2_PATH": "fr", "SFM_L2FR_CERT": "0"}}


class OtherLib:
    """sfm_match_batch of another build of the library, on torch's current stream."""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        vp, i32 = C.c_void_p, C.c_int32
        self.lib.sfm_ctx_create.argtypes = [i32, C.POINTER(vp)]
        self.lib.sfm_ctx_set_stream.argtypes = [vp, vp]
        self.lib.sfm_match_batch.argtypes = [vp, vp, vp, i32, i32, i32, vp, i32,
                                             C.POINTER(sfmcore.MatchParams), vp, vp, vp]
        self.h = vp()
        assert self.lib.sfm_ctx_create(0, C.byref(self.h)) == 0
        s = torch.cuda.current_stream(0).cuda_stream
        assert self.lib.sfm_ctx_set_stream(self.h, vp(s)) == 0

    def match(self, desc, n_kp, pairs, out):
        n_img, k_max, dim = desc.shape
        prm = sfmcore.MatchParams(0, sfmcore.XC_MUTUAL, 4, 5, -1)
        rc = self.lib.sfm_match_batch(self.h, desc.data_ptr(), n_kp.data_ptr(), n_img, k_max, dim,
                                      pairs.data_ptr(), pairs.shape[0], C.byref(prm),
                                      out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
        assert rc == 0
        return out


def main():
    r, n = (int(x) for x in os.environ.get("SHARD", "3/8").split("/"))
    rounds = int(os.environ.get("ROUNDS", "6"))
    n_img, k = int(os.environ.get("N_IMG", "500")), int(os.environ.get("K", "4096"))
    s = synth.make_scene(n_img, k, seed=0)
    pairs = synth.unordered_pairs(n_img)
    lo, hi = match_graph.shard_range(pairs, r, n, s["n_kp"])
    pairs = pairs[lo:hi]
    ctx = sfmcore.context(0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    desc, n_kp, pr = T(s["desc"]), T(s["n_kp"]), T(pairs)
    parent = OtherLib(os.environ["PARENT_LIB"]) if os.environ.get("PARENT_LIB") else None
    legs = os.environ.get("LEGS", "parent,mutual,cert,fr_rev").split(",")
    legs = [l for l in legs if l != "parent" or parent]
    os.environ.pop("SFM_L2_PATH", None)

    def call(leg, out):
        if leg == "parent":
            return parent.match(desc, n_kp, pr, out)
        return ctx.match_batch(desc, n_kp, pr, cross_check=sfmcore.XC_MUTUAL, ratio=(4, 5), out=out)
    P, km = len(pairs), desc.shape[1]
    bufs = {l: (torch.empty(P, dtype=torch.int32, device="cuda"),
                torch.empty((P, km, 2), dtype=torch.int32, device="cuda"),
                torch.empty((P, km), dtype=torch.int32, device="cuda")) for l in legs}
    times = {l: [] for l in legs}
    warm = int(os.environ.get("WARMUP", "1"))   # untimed rounds first (clocks, caches, workspaces)
    # a sample = REPS back-to-back calls between two events, reported per call: a window of one
    # sub-millisecond call measures the clock ramp as much as the kernels.  Default: enough calls
    # for about 50 ms per sample, sized from the slowest leg's warm-up call (1 without warm-up).
    reps, slowest = int(os.environ.get("REPS", "0")), 0.0
    for rnd in range(warm + rounds):
        if rnd == warm and reps < 1:
            reps = max(1, int(np.ceil(50.0 / slowest))) if slowest > 0 else 1
        for leg in legs:
            for kk, v in ENV.get(leg, {}).items():
                os.environ[kk] = v
            call(leg, bufs[leg])
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(reps if rnd >= warm else 1):
                call(leg, bufs[leg])
            ev[1].record()
            torch.cuda.synchronize()
            if rnd >= warm:
                times[leg].append(ev[0].elapsed_time(ev[1]) / reps)
            else:
                slowest = max(slowest, ev[0].elapsed_time(ev[1]))
            for kk in ENV.get(leg, {}):
                os.environ.pop(kk, None)
    ctx.match_cert_stats(enable=True)
    os.environ.update(ENV["cert"])
    call("cert", bufs["cert"])
    stats = ctx.match_cert_stats(enable=False, read=True)
    os.environ.pop("SFM_L2_PATH", None)
    cnt = {l: bufs[l][0].cpu().numpy() for l in legs}
    base = legs[0]
    same = all(bool((cnt[l] == cnt[base]).all()) for l in legs)
    if same:   # compare the rows each pair wrote (the rest of the buffers is never written)
        live = torch.arange(km, device="cuda")[None, :] < bufs[base][0][:, None]
        for l in legs[1:]:
            same &= bool((bufs[l][1][live] == bufs[base][1][live]).all())
            same &= bool((bufs[l][2][live] == bufs[base][2][live]).all())
    res = {"shard": f"{r}/{n}", "pairs": int(P), "n_img": n_img, "k": k, "rounds": rounds,
           "warmup_rounds": warm, "calls_per_sample": reps,
           "ms": times, "mean_ms": {l: float(np.mean(t)) for l, t in times.items()},
           "spread_ms": {l: float(max(t) - min(t)) for l, t in times.items()},
           "matches": int(cnt[base].sum()), "bit_identical": same,
           "cert_stats": dict(zip(("certified", "flagged", "exact_dots"), stats))}
    ref = "parent" if parent else "mutual"
    if ref in times and "cert" in times:
        gain = res["mean_ms"][ref] - res["mean_ms"]["cert"]
        margin = 3 * max(res["spread_ms"][ref], res["spread_ms"]["cert"])
        res["verdict"] = {"baseline": ref, "gain_ms": gain, "margin_ms": margin,
                          "keep_new_default": bool(gain > margin)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
