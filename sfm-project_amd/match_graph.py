"""Batched match + verify over an image-pair list, sharded across GPUs.

This is the reference's pair loop (code/pipeline.py:36-49: for every image pair, extract_and_match,
keep non-empty results as Pair(img_inx_1, img_inx_2, matches)) restated for one process per GPU:

* the unordered pair list (a<b) is cut into contiguous shards balanced by cost Ka*Kb;
* each rank runs K1 (MFMA matcher) and K2 (RANSAC) on its shard — no collective on the data path;
  RANSAC is keyed by (seed, a, b, h), so every pair's result is independent of the sharding;
* the verified match graph (the analogue of `pair_matches`) is exchanged once with two
  all-gathers over RCCL (`nccl` backend) — or gloo for the CPU tests: per-pair row counts, then
  the rows packed to 4 B ((queryIdx << 16) | trainIdx; the pair index is implied by the counts
  and the deterministic shard ranges), 3x less xGMI traffic than (pair, q, t) int32 rows.
"""
from __future__ import annotations

import numpy as np

import sfmcore


def shard_range(pairs: np.ndarray, rank: int, world: int, n_kp=None):
    """[lo, hi) of the contiguous shard `rank`, balanced by the per-pair cost n_kp[a]*n_kp[b]."""
    pairs = np.asarray(pairs, np.int32)
    if world <= 1:
        return 0, len(pairs)
    if n_kp is None:
        cost = np.ones(len(pairs))
    else:
        n_kp = np.asarray(n_kp, np.float64)
        cost = n_kp[pairs[:, 0]] * n_kp[pairs[:, 1]] + 1.0
    cum = np.concatenate([[0.0], np.cumsum(cost)])
    cuts = np.searchsorted(cum, cum[-1] * np.arange(world + 1) / world, side="left")
    cuts[0], cuts[-1] = 0, len(pairs)
    cuts = np.maximum.accumulate(cuts)
    return int(cuts[rank]), int(cuts[rank + 1])


def shard_pairs(pairs: np.ndarray, rank: int, world: int, n_kp=None) -> np.ndarray:
    lo, hi = shard_range(pairs, rank, world, n_kp)
    return np.asarray(pairs, np.int32)[lo:hi]


# Guided matching defaults: a 4 px^2 Sampson band (2 px), Lowe 4/5 inside the band, the mutual
# rule, and COLMAP's descriptor cap 0.7 on unit descriptors at this project's 512 scale,
# (0.7 * 512)^2 = 128450.  The cap matters: a query with a single candidate in its band passes the
# ratio test automatically.
GUIDED_DEFAULTS = dict(thr=4.0, ratio=(4, 5), cross_check=sfmcore.XC_MUTUAL, max_dist=128450)


def guided_options(guided):
    """None for off (None / False), else GUIDED_DEFAULTS updated by the caller's dict."""
    if guided is None or guided is False:
        return None
    kw = dict(GUIDED_DEFAULTS)
    if guided is not True:
        extra = set(guided) - set(kw)
        if extra:
            raise ValueError(f"guided: unknown option(s) {sorted(extra)}; known: {sorted(kw)}")
        kw.update(guided)
    return kw


class GraphBuilder:
    """Holds one image set on the device and verifies pair batches against it."""

    def __init__(self, desc, kps, n_kp=None, device: int = 0, ratio=(4, 5),
                 cross_check=sfmcore.XC_MUTUAL, max_dist=-1, n_hyp=4096, seed=42, thr=1.0,
                 min_inliers=15, guided=None):
        """guided: None / False (the default: K1 + K2 only), True, or a dict of thr, ratio,
        cross_check, max_dist overriding GUIDED_DEFAULTS: run() then re-matches every verified
        pair inside the epipolar band of its F and verifies again."""
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", device)
        self.ctx = sfmcore.context(device)
        desc = np.ascontiguousarray(desc, np.uint8)
        self.n_img, self.k_max, self.dim = desc.shape
        if n_kp is None:
            n_kp = np.full(self.n_img, self.k_max, np.int32)
        self.desc = torch.from_numpy(desc).to(self.dev)
        self.kps = torch.from_numpy(np.ascontiguousarray(kps, np.float32)).to(self.dev)
        self.n_kp = torch.from_numpy(np.ascontiguousarray(n_kp, np.int32)).to(self.dev)
        self.metric = sfmcore.METRIC_L2 if self.dim == 128 else sfmcore.METRIC_HAMMING
        self.match_kw = dict(metric=self.metric, cross_check=cross_check, ratio=ratio,
                             max_dist=max_dist)
        self.ransac_kw = dict(n_hyp=n_hyp, seed=seed, thr=thr, min_inliers=min_inliers)
        self.min_inliers = min_inliers
        self.guided_kw = guided_options(guided)
        if self.guided_kw is not None and self.metric != sfmcore.METRIC_L2:
            raise ValueError("GraphBuilder: guided matching needs L2 (128-byte) descriptors")
        self._bufs = {}

    def _buffers(self, P):
        """Output buffers for a batch of P pairs, reused by every later call with the same P.

        match / verify / run return views of these buffers: a later call with the same P
        overwrites them (graph_rows copies what it keeps into a fresh tensor).  Up to four batch
        sizes stay cached, so a chunked pass (equal chunks + one ragged tail) allocates once."""
        b = self._bufs.pop(P, None)
        if b is None:
            torch, dev, K = self.torch, self.dev, self.k_max
            b = dict(match=(torch.empty(P, dtype=torch.int32, device=dev),
                            torch.empty((P, K, 2), dtype=torch.int32, device=dev),
                            torch.empty((P, K), dtype=torch.int32, device=dev)),
                     ransac=dict(inl_count=torch.empty(P, dtype=torch.int32, device=dev),
                                 best_h=torch.empty(P, dtype=torch.int32, device=dev),
                                 mask=torch.empty((P, K), dtype=torch.uint8, device=dev),
                                 F=torch.empty((P, 9), dtype=torch.float32, device=dev),
                                 norm=torch.empty((P, 6), dtype=torch.float32, device=dev)))
            while len(self._bufs) >= 4:
                self._bufs.pop(next(iter(self._bufs)))
        self._bufs[P] = b  # most recently used last
        return b

    def match(self, pairs_t):
        b = self._buffers(pairs_t.shape[0])
        return self.ctx.match_batch(self.desc, self.n_kp, pairs_t, out=b["match"],
                                    **self.match_kw)

    def verify(self, pairs_t, count, match):
        b = self._buffers(pairs_t.shape[0])
        return self.ctx.ransac_batch(self.kps, pairs_t, count, match, out=b["ransac"],
                                     **self.ransac_kw)

    def _guided_buffers(self, b, P):
        """The second buffer set of a batch size (guided matches and their verification),
        allocated the first time a guided run needs it."""
        if "guided" not in b:
            torch, dev, K = self.torch, self.dev, self.k_max
            b["guided"] = (torch.empty(P, dtype=torch.int32, device=dev),
                           torch.empty((P, K, 2), dtype=torch.int32, device=dev),
                           torch.empty((P, K), dtype=torch.int32, device=dev))
            b["guided_ransac"] = {k: torch.empty_like(v) for k, v in b["ransac"].items()}
        return b["guided"], b["guided_ransac"]

    def guided_match(self, pairs_t, rs):
        """Guided matches of a batch from its first verification `rs` (sfm_guided_match_batch on
        rs's F, norm and inl_count); a pair that did not verify gets count 0."""
        b = self._buffers(pairs_t.shape[0])
        out, _ = self._guided_buffers(b, pairs_t.shape[0])
        return self.ctx.guided_match_batch(self.desc, self.n_kp, self.kps, pairs_t,
                                           rs["inl_count"], rs["F"], rs["norm"], out=out,
                                           min_inliers=self.min_inliers, **self.guided_kw)

    def run(self, pairs_t):
        """K1 + K2 on one pair batch; returns (count, match, dist, ransac dict) device tensors.
        With guided matching on: K1, K2, the guided re-match on K2's F, then K2 again on the
        guided matches with the same seed and pair keys; the second pass's tensors are returned."""
        count, match, dist = self.match(pairs_t)
        rs = self.verify(pairs_t, count, match)
        if self.guided_kw is None:
            return count, match, dist, rs
        count, match, dist = self.guided_match(pairs_t, rs)
        b = self._buffers(pairs_t.shape[0])
        rs = self.ctx.ransac_batch(self.kps, pairs_t, count, match, out=b["guided_ransac"],
                                   **self.ransac_kw)
        return count, match, dist, rs

    def graph_rows(self, pair_base: int, count, match, rs, return_offsets=False, packed=False):
        """Verified inlier rows [n,3] int32 (global pair index, queryIdx, trainIdx), on device
        (sfm_graph_offsets + sfm_graph_rows); return_offsets: also the per-pair row offsets;
        packed: the exchange form [n] int32 queryIdx << 16 | trainIdx (sfm_graph_rows_packed)."""
        return self.ctx.graph_rows(pair_base, count, match, rs["inl_count"], rs["mask"],
                                   self.min_inliers, return_offsets=return_offsets,
                                   packed=packed)


def all_gather_rows(rows, group=None):
    """All-gather variable-length [n,3] int32 row blocks from every rank (rank order).

    Two collectives: the per-rank row count, then the rows padded to the maximum count (RCCL has
    no all-gatherv)."""
    import torch
    import torch.distributed as dist
    if not dist.is_available() or not dist.is_initialized():
        return rows
    world = dist.get_world_size(group)
    n = torch.tensor([rows.shape[0]], dtype=torch.int64, device=rows.device)
    ns = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(ns, n, group=group)
    counts = [int(x.item()) for x in ns]
    m = max(max(counts), 1)
    pad = torch.zeros((m, rows.shape[1]), dtype=rows.dtype, device=rows.device)
    pad[:rows.shape[0]] = rows
    if dist.get_backend(group) == "nccl":  # RCCL: one contiguous all-gather
        out = torch.empty((world * m, rows.shape[1]), dtype=rows.dtype, device=rows.device)
        dist.all_gather_into_tensor(out, pad, group=group)
        parts = [out[r * m:r * m + counts[r]] for r in range(world)]
    else:  # gloo (CPU tests)
        bufs = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(bufs, pad, group=group)
        parts = [bufs[r][:counts[r]] for r in range(world)]
    return torch.cat(parts)


def pack_rows(rows, offsets):
    """Device-side compact form of one rank's graph rows (pair-major, as graph_rows writes them):
    per-pair row counts [P] int32 (from the [P+1] offsets) and rows packed as
    (queryIdx << 16) | trainIdx int32 — 4 B per row instead of 12 (indices < 65536)."""
    counts = (offsets[1:] - offsets[:-1]).to(rows.dtype)
    packed = (rows[:, 1] << 16) | rows[:, 2]
    return counts, packed


def all_gather_graph(counts, packed, ranges, group=None):
    """All-gather the compact graph of every rank and expand it to [n,3] int32 rows
    (global pair, queryIdx, trainIdx) in rank order.

    `ranges` = [(lo, hi)] pair range of every rank (match_graph.shard_range, known to all ranks
    without communication).  Two collectives: the per-pair counts (padded to the longest shard),
    then the packed rows (padded to the largest row count).  No process group: local expansion
    only (an initialised group of size 1 still runs the collectives).  Device tensors expand in
    one kernel straight out of the padded gather buffer (sfm_graph_expand); host tensors (the
    gloo CPU rehearsals) with the same arithmetic in torch."""
    import torch
    import torch.distributed as dist
    dev = packed.device
    single = not dist.is_available() or not dist.is_initialized()
    if single:
        world, call, rall, maxn = 1, counts.reshape(1, -1), packed.reshape(1, -1), packed.shape[0]
        tot = [int(packed.shape[0])]
    else:
        world = dist.get_world_size(group)
        maxp = max(max(hi - lo for lo, hi in ranges), 1)
        cpad = torch.zeros(maxp, dtype=torch.int32, device=dev)
        cpad[:counts.shape[0]] = counts
        call = _gather(cpad, world, group)
        tot = call.sum(dim=1).tolist()
        maxn = max(max(tot), 1)
        rpad = torch.zeros(maxn, dtype=torch.int32, device=dev)
        rpad[:packed.shape[0]] = packed
        rall = _gather(rpad, world, group)
    return expand_gathered(call, rall, tot, ranges[:world], maxn)


def expand_gathered(call, rall, tot, ranges, maxn):
    """[n,3] int32 rows from a gathered packed graph: call [world, >= hi-lo] per-pair counts and
    rall [world, maxn] packed rows of every rank r (its pairs ranges[r] = (lo, hi), its tot[r]
    rows first in its slot).  Device tensors: one sfm_graph_expand launch; host tensors: torch."""
    import torch
    dev = rall.device
    world = len(ranges)
    spans = [(r, hi - lo) for r, (lo, hi) in enumerate(ranges)]
    if dev.type == "cuda":
        # pair p of rank r: its rows start at r * maxn + (exclusive scan of rank r's counts)
        incl = torch.cumsum(call.long(), dim=1)
        src_all = incl - call.long() + torch.arange(world, device=dev).reshape(-1, 1) * maxn
        cnt_g = torch.cat([call[r, :n] for r, n in spans]).to(torch.int32).contiguous()
        src_g = torch.cat([src_all[r, :n] for r, n in spans]).contiguous()
        dst_g = (torch.cumsum(cnt_g.long(), dim=0) - cnt_g.long()).contiguous()
        return sfmcore.context(dev.index).graph_expand(ranges[0][0], cnt_g, src_g, dst_g,
                                                       rall.reshape(-1).contiguous(), sum(tot))
    out = []
    for (lo, hi), (r, n) in zip(ranges, spans):
        c, pk = call[r, :n], rall[r, :tot[r]]
        pair = torch.repeat_interleave(torch.arange(lo, hi, device=dev, dtype=torch.int32),
                                       c.long(), output_size=pk.shape[0])
        out.append(torch.stack([pair, (pk >> 16) & 0xFFFF, pk & 0xFFFF], dim=1))
    return torch.cat(out)


def _gather(t, world, group):
    """all-gather of equal-size 1-D tensors -> [world, n] (RCCL: one contiguous collective)."""
    import torch
    import torch.distributed as dist
    if dist.get_backend(group) == "nccl":
        out = torch.empty((world, t.shape[0]), dtype=t.dtype, device=t.device)
        dist.all_gather_into_tensor(out.view(-1), t, group=group)
        return out
    tc = t.cpu()  # gloo (CPU tests, same-GPU rehearsal): host buffers
    bufs = [torch.empty_like(tc) for _ in range(world)]
    dist.all_gather(bufs, tc, group=group)
    return torch.stack(bufs).to(t.device)


def rows_to_pairs(rows: np.ndarray, pairs: np.ndarray):
    """Host view of a gathered graph: list of (a, b, [(queryIdx, trainIdx), ...]) like the
    reference's pair_matches (code/pipeline.py:43-47)."""
    out = []
    if len(rows) == 0:
        return out
    order = np.argsort(rows[:, 0], kind="stable")
    rows = rows[order]
    starts = np.flatnonzero(np.r_[True, rows[1:, 0] != rows[:-1, 0]])
    ends = np.r_[starts[1:], len(rows)]
    for s, e in zip(starts, ends):
        p = int(rows[s, 0])
        out.append((int(pairs[p, 0]), int(pairs[p, 1]), rows[s:e, 1:].copy()))
    return out


# ---- tracks (graph -> tracks -> triangulation / BA) ---------------------

def build_tracks(rows, pairs, n_kp, min_len: int = 2, device: int = 0):
    """Feature tracks of a verified match graph on the GPU (`sfm_tracks`).

    rows [n,3] (pair, queryIdx, trainIdx), pairs [P,2] (image a, image b), n_kp [n_img] keypoints
    per image (numpy or device tensors).  Returns (track_ptr [T+1], track_img [m], track_kp [m])
    int32 device tensors: track t observes keypoint track_kp[i] of image track_img[i] for
    i in [track_ptr[t], track_ptr[t+1]); at most one keypoint per image."""
    import torch
    dev = torch.device("cuda", device)
    T = lambda a: (a.to(dev, torch.int32).contiguous() if isinstance(a, torch.Tensor)
                   else torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev))
    n_kp = T(n_kp)
    img_base = torch.zeros(n_kp.shape[0] + 1, dtype=torch.int32, device=dev)
    img_base[1:] = torch.cumsum(n_kp, 0)
    return sfmcore.context(device).tracks(img_base, T(pairs).reshape(-1, 2),
                                          T(rows).reshape(-1, 3), min_len)


def tracks_to_observations(track_ptr, track_img, track_kp, kps):
    """BA observations of the tracks: (cam_idx = image, pt_idx = track, uv [m,2] f64) in
    point-major order, the layout sfm_ba_jtj / sfm_ba_solve take.  kps [n_img, K, 2] (device)."""
    import torch
    counts = track_ptr[1:] - track_ptr[:-1]
    pt_idx = torch.repeat_interleave(torch.arange(counts.shape[0], device=counts.device,
                                                  dtype=torch.int32), counts.long())
    uv = kps[track_img.long(), track_kp.long()].to(torch.float64)
    return track_img, pt_idx, uv


# ---- on-disk match graph ------------------------------------------------

GRAPH_FORMAT = "sfm-core match graph v1"


def save_graph(path: str, pairs: np.ndarray, rows: np.ndarray, n_kp=None, meta=None):
    """Write a verified match graph as .npz (no pickles): pairs [P,2] i32 (image a, image b),
    rows [n,3] i32 (pair index, queryIdx, trainIdx), optional per-image keypoint counts and a
    JSON metadata string (e.g. RANSAC seed / threshold, descriptor kind)."""
    import json
    np.savez_compressed(path, format=np.array(GRAPH_FORMAT),
                        pairs=np.ascontiguousarray(pairs, np.int32),
                        rows=np.ascontiguousarray(rows, np.int32),
                        n_kp=np.asarray([] if n_kp is None else n_kp, np.int32),
                        meta=np.array(json.dumps(meta or {})))


def load_graph(path: str):
    """Inverse of save_graph (allow_pickle stays False).  Returns dict(pairs, rows, n_kp, meta)
    and `pair_matches` = rows_to_pairs(rows, pairs)."""
    import json
    with np.load(path, allow_pickle=False) as z:
        if str(z["format"]) != GRAPH_FORMAT:
            raise ValueError(f"{path}: not a {GRAPH_FORMAT!r} file")
        out = dict(pairs=z["pairs"], rows=z["rows"], n_kp=z["n_kp"],
                   meta=json.loads(str(z["meta"])))
    out["pair_matches"] = rows_to_pairs(out["rows"], out["pairs"])
    return out
