"""The ratio path (forward scan + its tail: recovery, compaction, certificate) of this build
against the same path of another build of the library, interleaved in one process on one box,
outputs compared bit for bit on every pair:
  parent   PARENT_LIB=path: the parent commit's libsfmcore.so, loaded next to this one
  new      this build
Both legs run with SFM_L2_PATH=fr (the default dispatch for the bench rule at 1536 < k_max <= 4096
and for every ratio-only call).  RULE=mutual (mutual + ratio 4/5, the bench rule) or RULE=ratio
(ratio 4/5 alone, BASELINE cfg2).
python tests/perf/k1_tail_ab.py  (SHARD=r/n, ROUNDS, WARMUP, REPS, N_IMG, K, RULE override;
default: the 1/8 cfg4 shard of k1_mutual_ab.py; cfg3: N_IMG=50 K=2048 SHARD=0/1; cfg2: the same
with RULE=ratio).  `verdict`: the change is kept only if mean(parent) - mean(new) is more than three
times the larger of the two legs' spreads (max - min over the rounds).  Also prints the shares of
the query slots that are candidates and ratio survivors (RULE=ratio counts the survivors)."""
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

    def match(self, desc, n_kp, pairs, xc, out):
        n_img, k_max, dim = desc.shape
        prm = sfmcore.MatchParams(0, xc, 4, 5, -1)
        rc = self.lib.sfm_match_batch(self.h, desc.data_ptr(), n_kp.data_ptr(), n_img, k_max, dim,
                                      pairs.data_ptr(), pairs.shape[0], C.byref(prm),
                                      out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
        assert rc == 0
        return out


def main():
    r, n = (int(x) for x in os.environ.get("SHARD", "3/8").split("/"))
    rounds = int(os.environ.get("ROUNDS", "6"))
    n_img, k = int(os.environ.get("N_IMG", "500")), int(os.environ.get("K", "4096"))
    rule = os.environ.get("RULE", "mutual")
    xc = sfmcore.XC_MUTUAL if rule == "mutual" else sfmcore.XC_NONE
    s = synth.make_scene(n_img, k, seed=0)
    pairs = synth.unordered_pairs(n_img)
    lo, hi = match_graph.shard_range(pairs, r, n, s["n_kp"])
    pairs = pairs[lo:hi]
    ctx = sfmcore.context(0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    desc, n_kp, pr = T(s["desc"]), T(s["n_kp"]), T(pairs)
    parent = OtherLib(os.environ["PARENT_LIB"]) if os.environ.get("PARENT_LIB") else None
    legs = (["parent"] if parent else []) + ["new"]
    os.environ["SFM_L2_PATH"] = "fr"

    def call(leg, out):
        if leg == "parent":
            return parent.match(desc, n_kp, pr, xc, out)
        return ctx.match_batch(desc, n_kp, pr, cross_check=xc, ratio=(4, 5), out=out)
    P, km = len(pairs), desc.shape[1]
    bufs = {l: (torch.empty(P, dtype=torch.int32, device="cuda"),
                torch.empty((P, km, 2), dtype=torch.int32, device="cuda"),
                torch.empty((P, km), dtype=torch.int32, device="cuda")) for l in legs}
    times = {l: [] for l in legs}
    warm = int(os.environ.get("WARMUP", "1"))   # untimed rounds first (clocks, caches, workspaces)
    # a sample = REPS back-to-back calls between two events, reported per call (about 50 ms per
    # sample, sized from the slowest leg's warm-up call)
    reps, slowest = int(os.environ.get("REPS", "0")), 0.0
    for rnd in range(warm + rounds):
        if rnd == warm and reps < 1:
            reps = max(1, int(np.ceil(50.0 / slowest))) if slowest > 0 else 1
        for leg in legs:
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
    cnt = {l: bufs[l][0].cpu().numpy() for l in legs}
    base = legs[0]
    same = all(bool((cnt[l] == cnt[base]).all()) for l in legs)
    if same:   # compare the rows each pair wrote (the rest of the buffers is never written)
        live = torch.arange(km, device="cuda")[None, :] < bufs[base][0][:, None]
        for l in legs[1:]:
            same &= bool((bufs[l][1][live] == bufs[base][1][live]).all())
            same &= bool((bufs[l][2][live] == bufs[base][2][live]).all())
    # the tail's load: candidates (queries the interval test keeps) and ratio survivors, as shares
    # of the pairs' query slots; the ratio-only rule's output count IS the survivor count
    nk = s["n_kp"].astype(np.int64)
    slots = int(nk[pairs[:, 0]][nk[pairs[:, 1]] > 0].sum())
    out_r = ctx.match_batch(desc, n_kp, pr, cross_check=sfmcore.XC_NONE, ratio=(4, 5))
    survivors = int(out_r[0].sum().item())
    # candidates: the interval test restated on the dumped forward records (SFM_L2FR_DEBUG=1:
    # match = (e1, e2), dist = tile) of the first pairs
    ns = min(P, 2048)
    os.environ["SFM_L2FR_DEBUG"] = "1"
    dbg = ctx.match_batch(desc, n_kp, pr[:ns].contiguous(), cross_check=xc, ratio=(4, 5))
    os.environ.pop("SFM_L2FR_DEBUG")
    torch.cuda.synchronize()
    A = ((desc.to(torch.int64) - 128) ** 2).sum(2)[pr[:ns, 0].long()]      # [ns, km] |x'|^2
    e1, e2 = dbg[1][:, :, 0].to(torch.int64), dbg[1][:, :, 1].to(torch.int64)
    d1lo = torch.clamp(A - 2 * e1 - 1, min=0)
    real2 = e2 > -(1 << 23)
    keep = ~real2 | (25 * d1lo < 16 * (A - 2 * e2))
    na_s, nb_s = n_kp[pr[:ns, 0].long()], n_kp[pr[:ns, 1].long()]
    valid = (torch.arange(km, device="cuda")[None, :] < na_s[:, None]) & (nb_s[:, None] > 0)
    cand = int((valid & keep & (e1 != e2)).sum().item())
    slow = int((valid & keep & (e1 == e2)).sum().item())
    vs = int(valid.sum().item())
    res = {"candidate_share": cand / max(vs, 1), "slow_share": slow / max(vs, 1),
           "candidate_sample_pairs": ns, "rule": rule, "shard": f"{r}/{n}", "pairs": int(P), "n_img": n_img, "k": k,
           "rounds": rounds, "warmup_rounds": warm, "calls_per_sample": reps,
           "ms": times, "mean_ms": {l: float(np.mean(t)) for l, t in times.items()},
           "spread_ms": {l: float(max(t) - min(t)) for l, t in times.items()},
           "matches": int(cnt[base].sum()), "bit_identical": same,
           "query_slots": slots, "ratio_survivors": survivors,
           "survivor_share": survivors / max(slots, 1)}
    if rule == "mutual":
        ctx.match_cert_stats(enable=True)
        call("new", bufs["new"])
        stats = ctx.match_cert_stats(enable=False, read=True)
        res["cert_stats"] = dict(zip(("certified", "flagged", "exact_dots"), stats))
    if parent:
        gain = res["mean_ms"]["parent"] - res["mean_ms"]["new"]
        margin = 3 * max(res["spread_ms"]["parent"], res["spread_ms"]["new"])
        res["verdict"] = {"gain_ms": gain, "gain_frac": gain / res["mean_ms"]["parent"],
                          "margin_ms": margin, "keep": bool(gain > margin)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
