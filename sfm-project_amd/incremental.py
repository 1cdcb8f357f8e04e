"""Incremental structure from motion over the GPU core ("rest of incremental
SfM for cfg5" — the pipeline papers/schoenberger2016sfm.pdf §2.1-2.2 describes and the reference's
empty code/3d_reconstruction.py would hold).

Every per-element stage runs on the GPU through the C-ABI: all-pairs matching (K1), F RANSAC (K2),
verified-graph rows, tracks (`sfm_tracks`), triangulation (`sfm_triangulate`), batched next-view
registration (`sfm_register_batch`, P3P RANSAC + refinement) and Levenberg-Marquardt bundle
adjustment (`sfm_ba_jtj` / `sfm_ba_solve`).  The host does the orchestration: which images and
tracks enter the model.  The initial pair's essential-matrix fit and decomposition run on the host
by default (`relative_pose`: an 8-point fit on that pair's inliers and four triangulations per
candidate pair); `reconstruct(init_pair="pose")` uses their GPU counterpart instead, the batched
`sfm_two_view_pose_batch`, and ranks the candidate pairs by their triangulation angles.

Cameras: angle-axis, t, f, k1 with known intrinsics (f, k1, principal point) per image.
"""
from __future__ import annotations

import os

import numpy as np

import match_graph
import reconstruction
import retrieval as _retrieval
import sfmcore


def _undistort(xy, intr, iters=10):
    """Normalised, undistorted coordinates (the triangulation kernel's fixed-point spec)."""
    f, k1, cx, cy = intr
    xd = (np.asarray(xy, np.float64) - [cx, cy]) / f
    x = xd.copy()
    for _ in range(iters):
        x = xd / (1.0 + k1 * np.sum(x * x, axis=1, keepdims=True))
    return x


def _angle_axis(R):
    c = np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = 0.5 * np.linalg.norm(w)
    th = np.arctan2(s, c)
    return w * (th / (2.0 * s)) if s > 1e-12 else 0.5 * w


def relative_pose(x1, x2):
    """Pose (R, t), |t| = 1, of camera 2 w.r.t. camera 1 from normalised correspondences: linear
    essential matrix on all pairs, projected to the essential manifold; the four decompositions
    are returned for the cheirality vote."""
    A = np.stack([x2[:, 0] * x1[:, 0], x2[:, 0] * x1[:, 1], x2[:, 0],
                  x2[:, 1] * x1[:, 0], x2[:, 1] * x1[:, 1], x2[:, 1],
                  x1[:, 0], x1[:, 1], np.ones(len(x1))], 1)
    E = np.linalg.svd(A)[2][-1].reshape(3, 3)
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    out = []
    for R in (U @ W @ Vt, U @ W.T @ Vt):
        for t in (U[:, 2], -U[:, 2]):
            out.append((R, t / np.linalg.norm(t)))
    return out


class Reconstruction:
    def __init__(self, n_img):
        self.timings = {}          # wall seconds per stage (each stage ends in a device sync)
        self.cams = np.zeros((n_img, 8))
        self.registered = np.zeros(n_img, bool)
        self.pts_d = None          # device [n_tr, 3] f64 points and [n_tr] bool flags: the driver
        self.has_d = None          # keeps them on the GPU; .points / .has_point are host copies
        self.history = []
        self.ba_log = []           # per bundle adjustment: size, LM / CG iterations, PCG branch
        self.n_verified = 0        # rows of the verified match graph
        self.pairs = None          # [P,2] i32 image pairs that were matched and verified
        self.obs_d = None          # device (obs_track, timg, obs_xy) of the track observations
        self.gauge = None          # (reference camera, scale camera) of the initial pair
        self._tracks_d = None      # device (ptr, img, kp) of the tracks; host copies on first use
        self._tracks = None
        self.obs_ok_d = None       # reconstruct(triangulation="ransac"): device [n_obs] bool, the
        #                            observation is still believed; .obs_ok is the host copy
        self.split = None          # reconstruct(triangulation="ransac_split"): the keyword
        #                            arguments of triangulate_multi (max_points, min_views)
        self.n_split = 0           # tracks created out of later consensus sets

    @property
    def tracks(self):
        """(ptr [n_tr + 1], img [n_obs], kp [n_obs]) host arrays of the tracks (copied from the
        device on first use: the reconstruction itself never reads them on the host)."""
        if self._tracks is None and self._tracks_d is not None:
            self._tracks = tuple(t.cpu().numpy() for t in self._tracks_d)
        return self._tracks

    @tracks.setter
    def tracks(self, v):
        self._tracks, self._tracks_d = v, None

    @property
    def points(self):
        """[n_tr, 3] host copy of the track points (valid where has_point); read-only — the model
        lives in pts_d, so writing to a copy would be lost (write to pts_d instead).  The copy is
        cached until pts_d is replaced or changed in place (repeated reads cost one
        device-to-host copy, not one each)."""
        return self._host("pts", self.pts_d)

    @property
    def has_point(self):
        """[n_tr] bool host copy: the track has a triangulated point (read-only and cached, see
        points)."""
        return self._host("has", self.has_d)

    @property
    def obs_ok(self):
        """[n_obs] bool host copy of obs_ok_d (None under the default triangulation; read-only
        and cached, see points)."""
        return self._host("obs_ok", self.obs_ok_d)

    def _host(self, name, t):
        if t is None:
            return None
        key = (id(t), t.data_ptr(), t._version)   # _version: bumped by every in-place write
        cache = self.__dict__.setdefault("_host_cache", {})
        c = cache.get(name)
        if c is None or c[0] != key or c[2] is not t:
            c = (key, _host_copy(t), t)
            cache[name] = c
        return c[1]


def _host_copy(t):
    if t is None:
        return None
    a = t.cpu().numpy()
    a.setflags(write=False)
    return a


def _match_graph(gb, pairs, pairs_t, n_kp, group):
    """Verified graph rows [n,3] (global pair, queryIdx, trainIdx) and every pair's inlier count.
    Under an initialised torch.distributed group (one process per GPU) each rank matches and
    verifies its contiguous shard_range of the pairs and the packed graph is all-gathered (the
    bench's exchange); the rows come back in pair order, so the result is the
    single-process one, bit for bit."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    if world == 1:
        count, match, _, rs = gb.run(pairs_t)
        return gb.graph_rows(0, count, match, rs), rs["inl_count"].cpu().numpy()
    rank = dist.get_rank(group)
    ranges = [match_graph.shard_range(pairs, r, world, n_kp) for r in range(world)]
    lo, hi = ranges[rank]
    dev = pairs_t.device
    if hi > lo:
        count, match, _, rs = gb.run(pairs_t[lo:hi].contiguous())
        packed, offs = gb.graph_rows(lo, count, match, rs, return_offsets=True, packed=True)
        cnt = (offs[1:] - offs[:-1]).to(torch.int32)
        inl_loc = rs["inl_count"]
    else:  # more ranks than pairs
        cnt = torch.zeros(0, dtype=torch.int32, device=dev)
        packed = torch.zeros(0, dtype=torch.int32, device=dev)
        inl_loc = torch.zeros(0, dtype=torch.int32, device=dev)
    graph = match_graph.all_gather_graph(cnt, packed, ranges, group)
    maxp = max(max(h - l for l, h in ranges), 1)
    ipad = torch.full((maxp,), -1, dtype=torch.int32, device=dev)
    ipad[:hi - lo] = inl_loc
    iall = match_graph._gather(ipad, world, group)
    inl = torch.cat([iall[r, :h - l] for r, (l, h) in enumerate(ranges)])
    return graph, inl.cpu().numpy()


def track_observations(ptr, img, kp, kps):
    """The observation arrays of the tracks (torch tensors of one device): (track id int64, image
    int64, keypoint [n, 2] f64) per observation, track-major — from the tracks CSR (ptr [T + 1],
    img / kp [n]) and the keypoints kps [n_img, K, 2] (any float dtype; f64 is exact)."""
    import torch
    n_tr, n_obs = int(ptr.numel()) - 1, int(img.numel())
    img_l = img.long()
    otr = torch.repeat_interleave(torch.arange(n_tr, dtype=torch.int64, device=ptr.device),
                                  (ptr[1:] - ptr[:-1]).long(), output_size=n_obs)
    xy = kps.reshape(-1, 2)[img_l * kps.shape[1] + kp.long()].to(torch.float64)
    return otr, img_l, xy


def track_obs(otr, timg, n_tr, tracks, in_img):
    """Observations of `tracks` (ascending track ids) whose image is flagged in `in_img`, as the
    triangulation kernel's CSR: (o, ptr) with o the observation indices in track order, ascending
    within a track (the observation arrays are track-major), ptr [len(tracks) + 1] int32.  Torch
    tensors of one device (the GPU in the driver; the CPU in tests/test_host_cpu.py)."""
    import torch
    want = torch.zeros(n_tr, dtype=torch.bool, device=otr.device)
    want[tracks] = True
    o = torch.nonzero(want[otr] & in_img[timg]).squeeze(1)
    cnt = torch.zeros(n_tr, dtype=torch.int64, device=otr.device)   # index_add: no sizing sync
    sel = otr[o]
    cnt.index_add_(0, sel, torch.ones_like(sel))
    ptr = torch.zeros(len(tracks) + 1, dtype=torch.int32, device=otr.device)
    ptr[1:] = torch.cumsum(cnt[tracks], 0)
    return o, ptr


def registration_obs(otr, timg, has_point, registered, min_corr=30):
    """2-D/3-D correspondences of every unregistered image with >= min_corr of them: observations
    of triangulated tracks in unregistered images, grouped by image (ascending) and ascending
    observation index within an image.  Returns (sel, ids, cptr): the selected observations, the
    candidate images and their CSR offsets (ids and cptr are small and come back to the host)."""
    import torch
    cand = torch.nonzero(has_point[otr] & ~registered[timg]).squeeze(1)
    img_sorted, by_img = torch.sort(timg[cand], stable=True)
    img_u, img_n = torch.unique_consecutive(img_sorted, return_counts=True)
    keep = img_n >= min_corr
    sel = cand[by_img][torch.repeat_interleave(keep, img_n)]
    n_keep = img_n[keep]
    cptr = torch.zeros(len(n_keep) + 1, dtype=torch.int64, device=otr.device)
    cptr[1:] = torch.cumsum(n_keep, 0)
    return sel, img_u[keep].cpu().numpy().astype(np.int32), cptr.cpu().numpy().astype(np.int32)


def point_mean(err, first):
    """Mean of `err` over each run of observations (runs start where `first` is set; every point's
    observations are contiguous), summed left to right within a run — the additions of
    numpy.bincount(pt_idx, err) / max(count, 1), so the same doubles — on the device: one
    masked gather-add per observation rank (tracks are short) instead of a host round trip."""
    import torch
    n_obs = err.shape[0]
    starts = torch.nonzero(first).squeeze(1)
    lens = torch.diff(starts, append=torch.tensor([n_obs], device=err.device))
    acc = torch.zeros(starts.shape[0], dtype=err.dtype, device=err.device)
    for k in range(int(lens.max()) if n_obs else 0):
        take = err[torch.clamp(starts + k, max=n_obs - 1)]
        acc = torch.where(lens > k, acc + take, acc)
    return acc / torch.clamp(lens, min=1).to(err.dtype)


def reconstruct(desc, kps, n_kp, intr, min_track=2, n_hyp=1024, reg_thr=4.0, max_err=4.0,
                ba_iter=20, loss_s=2.0, device=0, log=None, group=None, shard_ba=False,
                ba_cg_tol=0.1, ba_pcg="auto", ba_ftol=1e-6, init_pair="inliers",
                init_candidates=64, triangulation="dlt", pairs=None, retrieval=None,
                guided=None, split=None):
    """desc [n_img,K,D] u8, kps [n_img,K,2] pixels, n_kp [n_img], intr [n_img,4] = (f, k1, cx, cy).
    Returns a Reconstruction (cams [n_img,8], registered mask, points per track, track arrays).
    With torch.distributed initialised (one process per GPU, `group` or the default group) the
    all-pairs matching + verification is sharded across the ranks and the graph all-gathered; the
    later stages are deterministic, so every rank returns the single-process reconstruction.
    shard_ba additionally shards every bundle adjustment by point (reconstruction.bundle_adjust
    shard=True: camera-block and per-CG-iteration all-reduces); the ranks then still agree with
    each other exactly, and with the single-process run up to the fp64 summation order.
    ba_cg_tol: relative residual at which each LM step's Schur-complement PCG stops (Ceres'
    ITERATIVE_SCHUR forcing default, eta = 0.1): an inexact Newton step.  At 500 x 4096 the
    final BA takes 333 CG iterations instead of 3640 (1e-10) for the same optimum to 1e-7 of
    the cost and the same reconstruction.
    ba_pcg: the sharded bundle adjustments' PCG branch (reconstruction.bundle_adjust `pcg`:
    auto | sharded | replicated); rec.ba_log records the branch each one took.
    ba_ftol: an LM run stops once an accepted step lowers the cost by <= ba_ftol * cost (Ceres'
    and COLMAP's function tolerance, 1e-6); at 1e-12 every bundle adjustment of the 500-image
    cfg5 scene ran its 20 steps.
    init_pair: how the initial pair is chosen.  "inliers" (the default): the ten pairs with the
    most verified inliers in turn, each under the host's four essential-matrix decompositions.
    "pose": the `init_candidates` pairs with the most inliers go through the GPU pose batch
    (sfm_two_view_pose_batch) and are tried by descending n_wide, the number of inliers whose
    triangulation angle exceeds 2 degrees, each under the batch's winning pose only — on a dense
    sequence the most-matched pairs are the narrowest ones (_initial_pair_by_pose).
    triangulation: "dlt" (the default): every observation of a track enters its point, and the
    track stands or falls as a whole.  "ransac": sfm_triangulate_robust (RANSAC over the track's
    view pairs, keyed by the track id, threshold max_err) finds the observations that agree;
    rec.obs_ok_d / rec.obs_ok flag the observations still believed: one excluded by the
    triangulation's mask, or left above max_err by a bundle adjustment, stays out of the later
    adjustments, and a point with fewer than two believed observations in registered images is
    dropped.  "ransac_split": as "ransac", and sfm_triangulate_multi runs the RANSAC
    again on the observations outside the consensus set (`split`: a dict of its max_points,
    default 3, and min_views, default 2): a later consensus set that passes the acceptance test
    of a new point becomes a track of its own with that point, ids continuing after the existing
    tracks; rec.n_split counts them (a track that a wrong match merged out of two scene points
    gives both).  rec.obs_d, rec.tracks, rec.points / has_point / obs_ok then cover the new tracks
    too, still track-major.
    pairs: which image pairs are matched and verified.  None (the default): all of them.
    "retrieval": the pairs retrieval.select_pairs picks from the descriptors (vocabulary words,
    idf-weighted histogram intersection, each image's k best neighbours), with
    `retrieval` a dict of its keyword arguments (k, n_words, seed, lloyd, vocab).  It takes
    128-byte (L2) and 32-byte (binary, Hamming) descriptors; on binary ones keep the default
    n_words or pass lloyd=2 (retrieval.py).  Or a caller's
    integer [P,2] array with 0 <= a < b < n_img, brought to sorted unique order.  The list is
    kept as rec.pairs and the time it took as rec.timings["select_pairs"]; it is deterministic,
    so under torch.distributed every rank computes the same list itself.
    guided: None (the default), True or a dict of thr / ratio / cross_check / max_dist: guided
    matching (match_graph.GraphBuilder's `guided`).  Every verified pair is
    re-matched inside the epipolar band of its F and verified again, and the graph is built from
    the second verification."""
    import time
    import torch
    if init_pair not in ("inliers", "pose"):
        raise ValueError(f"reconstruct: init_pair must be 'inliers' or 'pose', got {init_pair!r}")
    if triangulation not in ("dlt", "ransac", "ransac_split"):
        raise ValueError(f"reconstruct: triangulation must be 'dlt', 'ransac' or 'ransac_split', "
                         f"got {triangulation!r}")
    robust = triangulation != "dlt"
    dev = torch.device("cuda", device)
    ctx = sfmcore.context(device)
    say = log or (lambda *a: None)
    tim = {}

    def lap(key, t0):
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        tim[key] = tim.get(key, 0.0) + (t1 - t0)
        return t1

    tk = time.perf_counter()
    n_img = len(desc)
    intr = np.asarray(intr, np.float64)
    if pairs is None:
        pairs = np.stack(np.triu_indices(n_img, 1), axis=1).astype(np.int32)  # (a < b), a-major
    else:
        if isinstance(pairs, str):
            if pairs != "retrieval":
                raise ValueError(f"reconstruct: pairs must be None, 'retrieval' or a [P, 2] array, "
                                 f"got {pairs!r}")
            pairs = _retrieval.select_pairs(desc, n_kp, device=device, **(retrieval or {}))
        else:
            pairs = _retrieval.check_pairs(pairs, n_img)
        tk = lap("select_pairs", tk)
    gb = match_graph.GraphBuilder(desc, kps, n_kp, device=device, guided=guided)
    pairs_t = torch.from_numpy(pairs).to(dev)
    rows, inl = _match_graph(gb, pairs, pairs_t, n_kp, group)
    tk = lap("match_verify", tk)
    ptr_t, timg_t, tkp_t = match_graph.build_tracks(rows, pairs_t, n_kp, min_track, device)
    n_tr = int(ptr_t.numel()) - 1
    kps_np = np.asarray(kps)
    # the observation arrays, built on the device (every bundle adjustment, registration and
    # triangulation selects its observations there; the host numpy build of the 1.4 M cfg5
    # observations took ~25 ms): track id per observation, image, and the keypoint as f64 (exact
    # from the caller's dtype; the builder's f32 copy when that is the caller's)
    kps_d = gb.kps if kps_np.dtype == np.float32 else torch.from_numpy(
        np.ascontiguousarray(kps_np)).to(dev)
    obs_d = track_observations(ptr_t, timg_t, tkp_t, kps_d)
    say(f"graph: {len(rows)} verified matches, {n_tr} tracks")

    rec = Reconstruction(n_img)
    rec.obs_d = obs_d
    rec.timings = tim
    rec.n_verified = int(rows.shape[0])
    rec.pairs = pairs
    rec._tracks_d = (ptr_t, timg_t, tkp_t)
    tk = lap("tracks", tk)
    rec.pts_d = torch.zeros((n_tr, 3), dtype=torch.float64, device=dev)
    rec.has_d = torch.zeros(n_tr, dtype=torch.bool, device=dev)
    rec.cams[:, 6:8] = intr[:, :2]
    if robust:
        rec.obs_ok_d = torch.ones(obs_d[0].shape[0], dtype=torch.bool, device=dev)
    if triangulation == "ransac_split":
        rec.split = dict(dict(max_points=3, min_views=2), **(split or {}))

    # ---- initial pair: most verified inliers; relative pose from that pair's RANSAC-verified
    # matches (tracks may still carry a wrong observation), then its tracks are triangulated
    # rows are pair-major in pair order: a pair's rows are one slice (no host copy of the graph)
    pair_col = rows[:, 0].contiguous()
    order = np.argsort(-inl, kind="stable")
    if init_pair == "pose":
        _initial_pair_by_pose(rec, ctx, gb, pairs, pairs_t, order[:int(init_candidates)], intr,
                              n_tr, max_err, say)
    for p in (order[:10] if init_pair == "inliers" else ()):
        a, b = (int(v) for v in pairs[p])
        pv = torch.tensor([int(p)], dtype=pair_col.dtype, device=dev)
        lo = int(torch.searchsorted(pair_col, pv).item())
        hi = int(torch.searchsorted(pair_col, pv, right=True).item())
        r = rows[lo:hi].cpu().numpy()
        if len(r) < 50:
            continue
        xa = _undistort(kps_np[a, r[:, 1]].astype(np.float64), intr[a])
        xb = _undistort(kps_np[b, r[:, 2]].astype(np.float64), intr[b])
        ta, tb = obs_d[0][obs_d[1] == a], obs_d[0][obs_d[1] == b]
        common = torch.unique(ta[torch.isin(ta, tb)]).cpu().numpy()   # sorted, as intersect1d
        best = None
        for R, t in relative_pose(xa, xb):
            cams = rec.cams.copy()
            cams[a, :6] = 0.0
            cams[b, :3] = _angle_axis(R)
            cams[b, 3:6] = t
            pts, st = (t.cpu().numpy() for t in
                       _triangulate(ctx, cams, intr, [a, b], common, rec.obs_d, n_tr,
                                    robust_thr=max_err if robust else None)[:2])
            good = int(np.sum((st[:, 3] == 0) & (st[:, 0] < max_err)))
            if best is None or good > best[0]:
                best = (good, cams, pts, st)
        good, cams_b, pts, st = best
        ok = (st[:, 3] == 0) & (st[:, 0] < max_err) & (st[:, 1] > 1.0)
        # at least 30 points with a triangulation angle above 1 degree: a near-zero baseline
        # (neighbouring views of a dense sequence) cannot seed the model
        if good >= 30 and int(ok.sum()) >= 30:
            rec.cams = cams_b
            sel = torch.from_numpy(common[ok]).to(dev)
            rec.pts_d[sel] = torch.from_numpy(np.ascontiguousarray(pts[ok])).to(dev)
            rec.has_d[sel] = True
            rec.registered[[a, b]] = True
            rec.gauge = (a, b)
            say(f"initial pair ({a}, {b}): {len(r)} verified matches, {int(ok.sum())} points")
            break
    if not rec.registered.any():
        raise RuntimeError("reconstruct: no initial pair with enough well-conditioned matches")
    tk = lap("initial_pair", tk)
    _bundle(rec, intr, loss_s, ba_iter, max_err, device, shard_ba, group, ba_cg_tol, ba_pcg,
            ba_ftol)
    tk = lap("bundle_adjust", tk)
    tim["rounds"] = 0

    # ---- register, triangulate, adjust until no image can be added
    while not rec.registered.all():
        # 2-D/3-D correspondences of every unregistered image with >= 30 of them, grouped by
        # image (ascending) and ascending observation index within an image: one pass
        # (selected on the device from rec.obs_d: ~1.5 M observations at cfg5)
        otr_d, timg_d, oxy_d = rec.obs_d   # a split rebuilds them
        sel, ids, cptr = registration_obs(otr_d, timg_d, rec.has_d,
                                          torch.from_numpy(rec.registered).to(dev))
        if len(ids) == 0:
            break
        T = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)
        pts_d = rec.pts_d
        cams_r, cnt, _, _ = ctx.register_batch(T(cptr, np.int32), oxy_d[sel].contiguous(),
                                               pts_d[otr_d[sel]].contiguous(),
                                               T(intr[ids], np.float64), T(ids, np.int32),
                                               n_hyp=n_hyp, thr=reg_thr)
        cams_r, cnt = cams_r.cpu().numpy(), cnt.cpu().numpy()
        tk = lap("register", tk)
        tim["rounds"] += 1
        added = 0
        for j, i in enumerate(ids):
            if cnt[j] >= 30:
                rec.cams[i] = cams_r[j]
                rec.registered[i] = True
                added += 1
        say(f"registered {added} of {len(ids)} candidates, total {int(rec.registered.sum())}")
        if not added:
            break
        _triangulate_new(rec, ctx, intr, max_err)
        tk = lap("triangulate", tk)
        _bundle(rec, intr, loss_s, ba_iter, max_err, device, shard_ba, group, ba_cg_tol,
                ba_pcg, ba_ftol)
        tk = lap("bundle_adjust", tk)
    return rec


def _initial_pair_by_pose(rec, ctx, gb, pairs, pairs_t, cand, intr, n_tr, max_err, say):
    """reconstruct(init_pair="pose"): seeds rec from the candidate pairs `cand` (indices into
    `pairs`, most inliers first).  The candidates are matched and verified again as one small
    batch on this device (the RNG is keyed by the image ids, so the masks are the all-pairs
    pass's, on every rank of a distributed run), the pose batch gives each its winning (R, t) and
    n_wide, and the candidates are tried by descending n_wide (stable): status 0, then the
    acceptance test of the default mode under that one pose — at least 30 well-reprojected
    triangulated tracks, at least 30 of them above 1 degree.  rec.init_candidates lists
    dict(pair, inliers, n_wide, status) of every candidate (most inliers first) and
    rec.init_tried the pairs tried, in order; no camera is set if none passes."""
    import torch
    dev = pairs_t.device
    cand = np.asarray(cand, np.int64)
    rec.init_tried = []
    if len(cand) == 0:
        return
    sub_t = pairs_t[torch.from_numpy(cand).to(dev)].contiguous()
    count, match, _, rs = gb.run(sub_t)
    po = ctx.two_view_pose_batch(gb.kps, torch.from_numpy(np.ascontiguousarray(intr)).to(dev),
                                 sub_t, count, match, rs["mask"], rs["inl_count"],
                                 min_inliers=gb.min_inliers)
    stat, Rs, ts = (po[k].cpu().numpy() for k in ("stat", "R", "t"))
    inl = rs["inl_count"].cpu().numpy()
    rec.init_candidates = [dict(pair=(int(pairs[c, 0]), int(pairs[c, 1])), inliers=int(inl[j]),
                                n_wide=int(stat[j, 6]), status=int(stat[j, 0]))
                           for j, c in enumerate(cand)]
    for j in np.argsort(-stat[:, 6], kind="stable"):
        a, b = rec.init_candidates[j]["pair"]
        rec.init_tried.append((a, b))
        if stat[j, 0] != 0:
            continue
        ta, tb = rec.obs_d[0][rec.obs_d[1] == a], rec.obs_d[0][rec.obs_d[1] == b]
        common = torch.unique(ta[torch.isin(ta, tb)]).cpu().numpy()
        cams = rec.cams.copy()
        cams[a, :6] = 0.0
        cams[b, :3] = _angle_axis(Rs[j].reshape(3, 3))
        cams[b, 3:6] = ts[j]
        pts, st = (t.cpu().numpy() for t in
                   _triangulate(ctx, cams, intr, [a, b], common, rec.obs_d, n_tr,
                                robust_thr=max_err if rec.obs_ok_d is not None else None)[:2])
        good = int(np.sum((st[:, 3] == 0) & (st[:, 0] < max_err)))
        ok = (st[:, 3] == 0) & (st[:, 0] < max_err) & (st[:, 1] > 1.0)
        if good >= 30 and int(ok.sum()) >= 30:
            rec.cams = cams
            sel = torch.from_numpy(common[ok]).to(dev)
            rec.pts_d[sel] = torch.from_numpy(np.ascontiguousarray(pts[ok])).to(dev)
            rec.has_d[sel] = True
            rec.registered[[a, b]] = True
            rec.gauge = (a, b)
            say(f"initial pair ({a}, {b}) by pose: n_wide {int(stat[j, 6])}, "
                f"{int(ok.sum())} points")
            return


def _triangulate(ctx, cams, intr, imgs, tracks, obs_d, n_tr, robust_thr=None):
    """Triangulate `tracks` (ascending ids: host array or device tensor) from their observations
    in the images `imgs` (GPU kernel; the observations are selected on the device from obs_d =
    (obs_track, timg, obs_xy)).  Returns device (pts [n, 3], stats [n, 4]) f64 tensors.
    robust_thr (pixels): sfm_triangulate_robust keyed by the track ids instead; then returns
    (pts, stats, o, mask): the observations used (indices into obs_d) and their conform flags."""
    import torch
    otr_d, timg_d, oxy_d = obs_d
    dev = otr_d.device
    in_img = torch.zeros(len(cams), dtype=torch.bool, device=dev)
    in_img[torch.as_tensor(np.asarray(imgs, np.int64), device=dev)] = True
    tr = (tracks.long() if isinstance(tracks, torch.Tensor) else
          torch.as_tensor(np.asarray(tracks, np.int64), device=dev))
    o, ptr = track_obs(otr_d, timg_d, n_tr, tr, in_img)
    T = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)
    if robust_thr is not None:
        pts, st, mask, _ = ctx.triangulate_robust(T(cams, np.float64), T(intr[:, 2:4], np.float64),
                                                  ptr, timg_d[o].to(torch.int32),
                                                  oxy_d[o].contiguous(), tr.to(torch.int32),
                                                  thr=robust_thr)
        return pts, st, o, mask
    return ctx.triangulate(T(cams, np.float64), T(intr[:, 2:4], np.float64), ptr,
                           timg_d[o].to(torch.int32), oxy_d[o].contiguous())


def _triangulate_new(rec, ctx, intr, max_err):
    """Triangulate every track without a point that has >= 2 observations in registered images."""
    import torch
    otr_d, timg_d, _ = rec.obs_d
    dev = otr_d.device
    n_tr = int(rec.has_d.numel())
    reg_d = torch.from_numpy(rec.registered).to(dev)
    n_reg = torch.zeros(n_tr, dtype=torch.int64, device=dev)
    sel = otr_d[reg_d[timg_d]]
    n_reg.index_add_(0, sel, torch.ones_like(sel))
    todo_d = torch.nonzero(~rec.has_d & (n_reg >= 2)).squeeze(1)
    if rec.split is not None:
        _triangulate_split(rec, ctx, intr, max_err, todo_d, reg_d)
        return
    if todo_d.numel() == 0:
        return
    if rec.obs_ok_d is not None:
        pts, st, o, mask = _triangulate(ctx, rec.cams, intr, np.nonzero(rec.registered)[0],
                                        todo_d, rec.obs_d, n_tr, robust_thr=max_err)
        ok = (st[:, 3] == 0) & (st[:, 0] < max_err) & (st[:, 1] > 1.0)
        rec.pts_d[todo_d[ok]] = pts[ok]
        rec.has_d[todo_d[ok]] = True
        # an accepted track's observations (all in registered images) that its point excludes
        acc = torch.zeros(n_tr, dtype=torch.bool, device=dev)
        acc[todo_d] = ok
        rec.obs_ok_d[o] = rec.obs_ok_d[o] & ~(acc[otr_d[o]] & (mask == 0))   # no sizing sync
        return
    pts, st = _triangulate(ctx, rec.cams, intr, np.nonzero(rec.registered)[0], todo_d, rec.obs_d,
                           n_tr)
    ok = (st[:, 3] == 0) & (st[:, 0] < max_err) & (st[:, 1] > 1.0)
    rec.pts_d[todo_d[ok]] = pts[ok]
    rec.has_d[todo_d[ok]] = True


def _triangulate_split(rec, ctx, intr, max_err, todo_d, reg_d):
    """_triangulate_new under triangulation="ransac_split", through sfm_triangulate_multi.
    1. The tracks todo_d (no point yet).  Slot 0 is handled as "ransac" handles its result.  Where
       it is accepted, a slot r >= 1 that passes the same test (status 0, error < max_err, ray
       angle > 1 degree) becomes a new track with that point: the observations labelled r move
       to it.  What is left of an accepted track's observations in registered images (label -1
       or a rejected slot) is no longer believed.
    2. The tracks that had a point before (the initial pair's among them, which step 1 never
       sees): their observations in registered images that the point does not explain (behind
       the camera or off by max_err or more) are a sub-track of their own, and every slot of it
       that passes the test becomes a new track."""
    import torch
    dev = reg_d.device
    T = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)
    cams_d, pp_d = T(rec.cams, np.float64), T(intr[:, 2:4], np.float64)
    had_d = rec.has_d.clone()

    def multi(tracks_d, o, ptr):
        otr_d, timg_d, oxy_d = rec.obs_d
        pts, st, _, _, label = ctx.triangulate_multi(cams_d, pp_d, ptr, timg_d[o].to(torch.int32),
                                                     oxy_d[o].contiguous(),
                                                     tracks_d.to(torch.int32), thr=max_err,
                                                     **rec.split)
        ok = (st[:, :, 3] == 0) & (st[:, :, 0] < max_err) & (st[:, :, 1] > 1.0)   # [n, R]
        # per observation of o: its row of the call and its label
        pos = torch.full((int(rec.has_d.numel()),), -1, dtype=torch.int64, device=dev)
        pos[tracks_d] = torch.arange(tracks_d.numel(), device=dev)
        return pts, ok, pos[otr_d[o]], label.long()

    def spawn(new, pts, o, row, lab):
        """The slots flagged in new [n, R] become tracks; returns the observations moved."""
        moved = (lab >= 0) & new[row, lab.clamp(min=0)]
        n_new = int(new.sum())                                  # the one sizing sync
        if n_new:
            n_tr = int(rec.has_d.numel())
            slot_id = torch.full(new.shape, -1, dtype=torch.int64, device=dev)
            slot_id[new] = n_tr + torch.arange(n_new, device=dev)   # (parent id, round) order
            rec.obs_ok_d[o[moved]] = True
            _move_observations(rec, o[moved], slot_id[row[moved], lab[moved]], pts[new])
            rec.n_split += n_new

    if todo_d.numel():
        n_tr = int(rec.has_d.numel())
        o, ptr = track_obs(rec.obs_d[0], rec.obs_d[1], n_tr, todo_d, reg_d)
        pts, ok, row, lab = multi(todo_d, o, ptr)
        ok0 = ok[:, 0]
        rec.pts_d[todo_d[ok0]] = pts[ok0, 0]
        rec.has_d[todo_d[ok0]] = True
        new = ok & ok0[:, None]
        new[:, 0] = False
        moved = (lab >= 1) & new[row, lab.clamp(min=0)]
        rec.obs_ok_d[o] = rec.obs_ok_d[o] & ~(ok0[row] & (lab != 0) & ~moved)   # no sizing sync
        spawn(new, pts, o, row, lab)

    otr_d, timg_d, oxy_d = rec.obs_d
    n_tr = int(rec.has_d.numel())
    had = torch.zeros(n_tr, dtype=torch.bool, device=dev)
    had[:had_d.numel()] = had_d & rec.has_d[:had_d.numel()]
    cand = torch.nonzero(had[otr_d] & reg_d[timg_d]).squeeze(1)
    err, depth = _reprojection(cams_d, pp_d, rec.pts_d[otr_d[cand]], timg_d[cand], oxy_d[cand])
    o = cand[~((depth > 0) & (err < max_err))]
    cnt = torch.zeros(n_tr, dtype=torch.int64, device=dev)
    cnt.index_add_(0, otr_d[o], torch.ones_like(o))
    tracks_d = torch.nonzero(cnt >= 2).squeeze(1)
    if tracks_d.numel() == 0:
        return
    o = o[cnt[otr_d[o]] >= 2]
    ptr = torch.zeros(tracks_d.numel() + 1, dtype=torch.int32, device=dev)
    ptr[1:] = torch.cumsum(cnt[tracks_d], 0)
    pts, ok, row, lab = multi(tracks_d, o, ptr)
    spawn(ok, pts, o, row, lab)


def _reprojection(cams_d, pp_d, X, img, xy):
    """Device (error in pixels, depth) of the points X [n, 3] in the images img [n] against the
    keypoints xy [n, 2] under the full camera model (angle-axis, t, f, k1)."""
    import torch
    c = cams_d[img]
    w = c[:, :3]
    th = torch.linalg.norm(w, dim=1, keepdim=True)
    k = w / th.clamp(min=1e-30)
    P = (X * torch.cos(th) + torch.linalg.cross(k, X) * torch.sin(th)
         + k * (k * X).sum(1, keepdim=True) * (1.0 - torch.cos(th))) + c[:, 3:6]
    q = P[:, :2] / P[:, 2:3]
    g = 1.0 + c[:, 7:8] * (q * q).sum(1, keepdim=True)
    e = c[:, 6:7] * g * q + pp_d[img] - xy
    return torch.linalg.norm(e, dim=1), P[:, 2]


def _move_observations(rec, obs, track, new_pts):
    """Appends len(new_pts) tracks with the points new_pts and moves the observations `obs` to
    the tracks `track` (ids from the old track count on).  The observation arrays stay
    track-major and contiguous, which the rest of the driver relies on: a stable device sort by
    the new track id, applied to rec.obs_d, obs_ok_d and the tracks CSR; pts_d / has_d grow."""
    import torch
    otr_d, timg_d, oxy_d = rec.obs_d
    ptr_t, img_t, kp_t = rec._tracks_d
    n_all = int(rec.has_d.numel()) + int(new_pts.shape[0])
    otr_new = otr_d.clone()
    otr_new[obs] = track
    otr_new, order = torch.sort(otr_new, stable=True)
    rec.obs_d = (otr_new, timg_d[order], oxy_d[order])
    rec.obs_ok_d = rec.obs_ok_d[order]
    ptr_new = torch.zeros(n_all + 1, dtype=ptr_t.dtype, device=ptr_t.device)
    ptr_new[1:] = torch.cumsum(torch.bincount(otr_new, minlength=n_all), 0)
    rec._tracks_d, rec._tracks = (ptr_new, img_t[order], kp_t[order]), None
    rec.pts_d = torch.cat([rec.pts_d, new_pts])
    rec.has_d = torch.cat([rec.has_d, torch.ones(new_pts.shape[0], dtype=torch.bool,
                                                 device=rec.has_d.device)])


def _bundle(rec, intr, loss_s, ba_iter, max_err, device, shard_ba=False, group=None, cg_tol=0.1,
            pcg="auto", ftol=1e-6):
    """Global LM over the registered cameras and the triangulated points (GPU), then drop points
    whose mean reprojection error stays above max_err.  Gauge: the initial pair's first camera
    keeps its pose and the second one translation coordinate (the scale); the intrinsics are
    known, so f and k1 are held too (reconstruction.gauge_mask).  The observations are selected
    on the device from rec.obs_d = (obs_track, timg, obs_xy)."""
    import time
    import torch
    t0 = time.perf_counter()
    otr_d, timg_d, oxy_d = rec.obs_d
    dev = otr_d.device
    reg_d = torch.from_numpy(rec.registered).to(dev)
    sel_d = reg_d[timg_d] & rec.has_d[otr_d]
    if rec.obs_ok_d is not None:
        sel_d &= rec.obs_ok_d
    use = torch.nonzero(sel_d).squeeze(1)   # the one sizing sync
    n_use = int(use.shape[0])
    if n_use == 0:
        return
    ref, second = rec.gauge
    fixed = reconstruction.gauge_mask(rec.cams, ref=ref, second=second, fix_intrinsics=True)
    # the registered cameras only, renumbered 0 .. n_reg - 1 in image order (an unregistered
    # camera has no observation here: it only added an empty block row to every kernel's camera
    # side — 500 camera blocks per setup at the first bundle adjustment of two views)
    reg_idx = np.nonzero(rec.registered)[0]
    timg_use = timg_d[use]
    if os.environ.get("SFM_BA_COMPACT", "1") != "0":
        remap = torch.full((len(rec.registered),), -1, dtype=torch.int32, device=dev)
        remap[torch.from_numpy(reg_idx).to(dev)] = torch.arange(len(reg_idx), dtype=torch.int32,
                                                                device=dev)
        ba_cams, ba_pp, ba_fixed = rec.cams[reg_idx], intr[reg_idx, 2:4], fixed[reg_idx]
        cam_sel = remap[timg_use.long()]
    else:
        reg_idx = None
        ba_cams, ba_pp, ba_fixed = rec.cams, intr[:, 2:4], fixed
        cam_sel = timg_use.to(torch.int32)
    tr = otr_d[use]   # non-decreasing (track-major): unique tracks by run starts
    first = torch.ones(n_use, dtype=torch.bool, device=dev)
    first[1:] = tr[1:] != tr[:-1]
    pts_ids = tr[first]     # device: the BA's points, gathered and scattered on the GPU
    pt_idx_d = torch.cumsum(first, 0, dtype=torch.int32) - 1
    info = {}
    t_sel = time.perf_counter() - t0    # observation selection (ends in host syncs)
    cams, pts, hist = reconstruction.bundle_adjust(ba_cams, ba_pp, rec.pts_d[pts_ids],
                                                   cam_sel, pt_idx_d,
                                                   oxy_d[use], loss_s=loss_s, max_iter=ba_iter,
                                                   cg_tol=cg_tol, ftol=ftol, device=device,
                                                   fixed=ba_fixed, shard=shard_ba, group=group,
                                                   pcg=pcg, info=info, reproj_err="device",
                                                   device_out=True)
    err_d = info.pop("err")   # device, at the returned parameters (bundle_adjust reproj_err)
    rec.ba_log.append(dict(info, n_cam=int(rec.registered.sum()), n_pt=int(pts_ids.numel()),
                           n_obs=n_use, lm_steps=len(hist),
                           lm_rejected=int(sum(1 for h in hist if not h[2])),
                           cg_iters=int(sum(h[3] for h in hist))))
    reg = rec.registered
    if reg_idx is not None:
        rec.cams[reg_idx] = cams
    else:
        rec.cams[reg] = cams[reg]
    rec.pts_d[pts_ids] = pts
    mean = point_mean(err_d, first)
    rec.has_d[pts_ids[mean > max_err]] = False
    if rec.obs_ok_d is not None:
        # an observation the adjusted model still misses by more than max_err is no longer
        # believed; a point left with fewer than two believed observations in registered
        # images goes (all on the device: no sync)
        rec.obs_ok_d[use] = ~(err_d > max_err)
        n_ok = torch.zeros(rec.has_d.numel(), dtype=torch.int64, device=dev)
        n_ok.index_add_(0, otr_d, (reg_d[timg_d] & rec.obs_ok_d).to(torch.int64))
        rec.has_d &= n_ok >= 2
    rec.ba_log[-1]["s"] = time.perf_counter() - t0   # setup + LM + reprojection filter
    rec.ba_log[-1]["select_s"] = t_sel
    rec.history.append((int(reg.sum()), int(rec.has_d.sum()),
                        float(hist[-1][0]) if hist else float("nan")))
