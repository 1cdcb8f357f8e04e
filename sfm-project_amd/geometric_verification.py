"""Fills the reference's empty code/geometric_verification.py (0 bytes; the pipeline's
"Geometric Verification" section at code/pipeline.py:60 is a bare comment).

`pipeline.py` star-imports this module (code/pipeline.py:3).  Verification is the build's spec
(after papers/schoenberger2016sfm.pdf §4.1): 8-point fundamental-matrix RANSAC,
`n_hyp` hypotheses per pair drawn by a counter-based RNG keyed (seed, a, b, h), Sampson error in
squared pixels below `thr`, best = max inlier count (lowest hypothesis id on ties); a pair is
verified when the count reaches `min_inliers`.  All arithmetic runs in libsfmcore (HIP).

Multi-model verification (the paper's §4.1): an F is not identifiable on a planar
scene or under pure rotation, yet such pairs pass the F test.  `verify_pair_h` /
`two_view_geometry` / `verify_pairs(homography=True)` also fit a homography by 4-point RANSAC
(sfm_ransac_h_batch) on the same tentative matches and `classify_two_view` compares the two inlier
counts.

Relative pose (the paper's §4.1-4.2): `two_view_pose` and
`verify_pairs(poses=True, intrinsics=...)` run the pose batch (sfm_two_view_pose_batch) on the F
inliers: a linear essential fit, its winning (R, t) by the cheirality vote, the number of inliers
in front of both cameras and their triangulation angle (`key_to_degrees`).

DEFAULT_H_THRESHOLD: the homography threshold is the forward transfer error |H x1 - x2|^2 in
squared pixels of image 2.  At sigma = 0.5 px per coordinate the F path's Sampson threshold of
1.0 px^2 keeps P(chi^2_1 < 4) = 0.954 of the true matches; the same share under the transfer error
(2 sigma^2 chi^2_2 with noise in both images) needs about 3.1 px^2, so 4.0 px^2 is the matching,
slightly more generous default.  DEFAULT_MAX_H_RATIO is COLMAP's max_H_inlier_ratio.
"""
from __future__ import annotations

import numpy as np

import sfmcore

DEFAULT_HYPOTHESES = 4096
DEFAULT_SEED = 42
DEFAULT_THRESHOLD = 1.0   # Sampson error, px^2
DEFAULT_MIN_INLIERS = 15  # COLMAP's default N_F
DEFAULT_H_THRESHOLD = 4.0  # forward transfer error, px^2 of image 2 (module docstring)
DEFAULT_MAX_H_RATIO = 0.8  # COLMAP's max_H_inlier_ratio
DEFAULT_MIN_ANGLE_DEG = 2.0  # a "wide" ray pair of the pose batch (n_wide)


def denormalize_F(Fn, norm) -> np.ndarray:
    """Pixel-space F = T2^T Fn T1 (fp64), unit Frobenius norm.  norm = (cx1,cy1,s1,cx2,cy2,s2)."""
    Fn = np.asarray(Fn, np.float64).reshape(3, 3)
    T1, T2 = _norm_transforms(norm)
    F = T2.T @ Fn @ T1
    n = np.linalg.norm(F)
    return F / n if n > 0 else F


def denormalize_H(Hn, norm) -> np.ndarray:
    """Pixel-space H = T2^-1 Hn T1 (fp64), unit Frobenius norm, sign fixed so that H[2,2] >= 0.
    norm = (cx1,cy1,s1,cx2,cy2,s2); a zero norm (a pair below 4 matches) gives the zero matrix."""
    Hn = np.asarray(Hn, np.float64).reshape(3, 3)
    T1, _ = _norm_transforms(norm)
    cx2, cy2, s2 = [float(v) for v in norm[3:6]]
    if s2 == 0.0:
        return np.zeros((3, 3))
    T2inv = np.array([[1.0 / s2, 0, cx2], [0, 1.0 / s2, cy2], [0, 0, 1.0]])
    H = T2inv @ Hn @ T1
    n = np.linalg.norm(H)
    H = H / n if n > 0 else H
    return -H if H[2, 2] < 0 else H


def _norm_transforms(norm):
    cx1, cy1, s1, cx2, cy2, s2 = [float(v) for v in norm]
    T1 = np.array([[s1, 0, -s1 * cx1], [0, s1, -s1 * cy1], [0, 0, 1.0]])
    T2 = np.array([[s2, 0, -s2 * cx2], [0, s2, -s2 * cy2], [0, 0, 1.0]])
    return T1, T2


def classify_two_view(f_count, h_count, min_inliers=DEFAULT_MIN_INLIERS,
                      max_h_ratio=DEFAULT_MAX_H_RATIO) -> str:
    """Two-view configuration from the F and H inlier counts on the same tentative matches:
    "unverified" when f_count < min_inliers; "planar_or_panoramic" when h_count >= min_inliers and
    h_count / f_count > max_h_ratio (the F is then not trustworthy: a planar scene or a pure
    rotation); "general" otherwise."""
    f_count, h_count = int(f_count), int(h_count)
    if f_count < min_inliers:
        return "unverified"
    if h_count >= min_inliers and _h_ratio(f_count, h_count) > max_h_ratio:
        return "planar_or_panoramic"
    return "general"


def _h_ratio(f_count, h_count) -> float:
    return max(int(h_count), 0) / int(f_count) if int(f_count) > 0 else 0.0


def key_to_degrees(key):
    """Ray angle in degrees of a pose-batch key (sfm_two_view_pose_batch: sin^2 of the angle up to
    90 degrees, 2 - sin^2 above; monotone over [0, 180])."""
    k = np.asarray(key, np.float64)
    lo = np.degrees(np.arcsin(np.sqrt(np.clip(k, 0.0, 1.0))))
    hi = 180.0 - np.degrees(np.arcsin(np.sqrt(np.clip(2.0 - k, 0.0, 1.0))))
    out = np.where(k <= 1.0, lo, hi)
    return float(out) if out.ndim == 0 else out


def _upload_pair(kp1, kp2, matches, pair, device, intr=None):
    """One pair as a 1-pair batch on the device: (ctx, kps, pairs, count, match, M).  The RNG is
    keyed by the pair's image ids, so they are passed through.  intr = (intr1, intr2): the
    per-image (f, k1, cx, cy) ride at the end of the int32 upload and come back as a seventh
    item, the [n_img, 4] f64 table."""
    import torch
    mt = _match_array(matches)
    k1, k2 = np.asarray(kp1, np.float32), np.asarray(kp2, np.float32)
    k_max = max(len(k1), len(k2), len(mt), 1)
    match = np.zeros((1, k_max, 2), np.int32)
    match[0, :len(mt)] = mt
    dev = torch.device("cuda", device)
    ctx = sfmcore.context(device)
    a, b = int(pair[0]), int(pair[1])
    n_img = max(a, b) + 1
    kps_full = np.zeros((n_img, k_max, 2), np.float32)
    kps_full[a, :len(k1)] = k1
    kps_full[b, :len(k2)] = k2
    # one int32 upload (pair, match count, 61 pad, matches)
    head = np.zeros(64, np.int32)
    head[:3] = (a, b, len(mt))
    parts = [head, match.reshape(-1)]
    if intr is not None:
        it = np.ones((n_img, 4), np.float64)   # f = 1 for the images that are not in the pair
        it[a], it[b] = np.asarray(intr[0], np.float64), np.asarray(intr[1], np.float64)
        parts.append(it.reshape(-1).view(np.int32))
    up = torch.from_numpy(np.concatenate(parts)).to(dev)
    n_mt = 64 + 2 * k_max    # even: the f64 view of the tail is aligned
    res = (ctx, torch.from_numpy(kps_full).to(dev), up[:2].view(1, 2), up[2:3],
           up[64:n_mt].view(1, k_max, 2), len(mt))
    if intr is not None:
        res += (up[n_mt:].view(torch.float64).view(n_img, 4),)
    return res


def _pack(out, model, M):
    """The first pair's results of a batch as one byte tensor: count, best_h, model, norm, mask."""
    import torch
    u8 = lambda t: t.reshape(-1).view(torch.uint8)
    return torch.cat([u8(out["inl_count"][:1]), u8(out["best_h"][:1]), u8(out[model][0]),
                      u8(out["norm"][0]), out["mask"][0, :M]])


def _unpack(back, M):
    cnt = int(back[0:4].view(np.int32)[0])
    best_h = int(back[4:8].view(np.int32)[0])
    model = back[8:44].view(np.float32).copy()
    norm = back[44:68].view(np.float32).copy()
    return cnt, best_h, model, norm, back[68:68 + M].astype(bool)


def verify_pair(kp1, kp2, matches, pair=(0, 1), n_hyp=DEFAULT_HYPOTHESES, seed=DEFAULT_SEED,
                thr=DEFAULT_THRESHOLD, min_inliers=DEFAULT_MIN_INLIERS, device=0):
    """kp1/kp2: [K,2] pixel coordinates; matches: list of DMatch or [M,2] (query, train) array.

    Returns dict(F [3,3] pixel F, inliers [n] match indices (ascending), count, verified,
    best_h)."""
    ctx, kps, pr, count, match, M = _upload_pair(kp1, kp2, matches, pair, device)
    out = ctx.ransac_batch(kps, pr, count, match, n_hyp=n_hyp, seed=seed, thr=thr,
                           min_inliers=min_inliers)
    # one byte download of the results
    cnt, best_h, Fn, norm, mask = _unpack(_pack(out, "F", M).cpu().numpy(), M)
    return dict(F=denormalize_F(Fn, norm), inliers=np.nonzero(mask)[0], count=max(cnt, 0),
                verified=cnt >= min_inliers, best_h=best_h)


def verify_pair_h(kp1, kp2, matches, pair=(0, 1), n_hyp=DEFAULT_HYPOTHESES, seed=DEFAULT_SEED,
                  thr=DEFAULT_H_THRESHOLD, min_inliers=DEFAULT_MIN_INLIERS, device=0):
    """The homography mirror of verify_pair (4-point RANSAC, forward transfer error below `thr`
    px^2 in image 2).  Returns dict(H [3,3] pixel H (unit norm, H[2,2] >= 0), inliers [n] match
    indices (ascending), count, verified, best_h)."""
    ctx, kps, pr, count, match, M = _upload_pair(kp1, kp2, matches, pair, device)
    out = ctx.ransac_h_batch(kps, pr, count, match, n_hyp=n_hyp, seed=seed, thr=thr,
                             min_inliers=min_inliers)
    cnt, best_h, Hn, norm, mask = _unpack(_pack(out, "H", M).cpu().numpy(), M)
    return dict(H=denormalize_H(Hn, norm), inliers=np.nonzero(mask)[0], count=max(cnt, 0),
                verified=cnt >= min_inliers, best_h=best_h)


def two_view_geometry(kp1, kp2, matches, pair=(0, 1), n_hyp=DEFAULT_HYPOTHESES,
                      seed=DEFAULT_SEED, thr=DEFAULT_THRESHOLD, h_thr=DEFAULT_H_THRESHOLD,
                      min_inliers=DEFAULT_MIN_INLIERS, max_h_ratio=DEFAULT_MAX_H_RATIO, device=0):
    """F and H RANSAC on the same tentative matches (one upload, the two batch calls, one
    download) and the configuration classify_two_view gives their counts.  Returns dict(config,
    F, H (pixel space), f_inliers, h_inliers (match indices), f_count, h_count, h_ratio)."""
    import torch
    ctx, kps, pr, count, match, M = _upload_pair(kp1, kp2, matches, pair, device)
    of = ctx.ransac_batch(kps, pr, count, match, n_hyp=n_hyp, seed=seed, thr=thr,
                          min_inliers=min_inliers)
    oh = ctx.ransac_h_batch(kps, pr, count, match, n_hyp=n_hyp, seed=seed, thr=h_thr,
                            min_inliers=min_inliers)
    back = torch.cat([_pack(of, "F", M), _pack(oh, "H", M)]).cpu().numpy()
    fc, _, Fn, fnorm, fmask = _unpack(back[:68 + M], M)
    hc, _, Hn, hnorm, hmask = _unpack(back[68 + M:], M)
    fc, hc = max(fc, 0), max(hc, 0)
    return dict(config=classify_two_view(fc, hc, min_inliers, max_h_ratio),
                F=denormalize_F(Fn, fnorm), H=denormalize_H(Hn, hnorm),
                f_inliers=np.nonzero(fmask)[0], h_inliers=np.nonzero(hmask)[0],
                f_count=fc, h_count=hc, h_ratio=_h_ratio(fc, hc))


def _pack_pose(po, p=0):
    """Pair p's pose-batch results as one byte tensor: E, R, t (21 f64), stat (8 i32), key (f32)."""
    import torch
    u8 = lambda t: t.reshape(-1).view(torch.uint8)
    return torch.cat([u8(po["E"][p]), u8(po["R"][p]), u8(po["t"][p]), u8(po["stat"][p]),
                      u8(po["median_key"][p:p + 1])])


_POSE_BYTES = 21 * 8 + 8 * 4 + 4


def _pose_fields(E, R, t, stat, key) -> dict:
    """The public pose fields from one pair's batch outputs (zero matrices unless status is 0)."""
    stat = [int(v) for v in stat]
    return dict(R=np.array(R, np.float64).reshape(3, 3), t=np.array(t, np.float64),
                E=np.array(E, np.float64).reshape(3, 3), n_front=stat[2 + stat[1]],
                n_front_all=stat[2:6], best=stat[1], tri_angle_deg=key_to_degrees(float(key)),
                n_wide=stat[6], status=stat[0])


def _unpack_pose(back) -> dict:
    f = back[:168].copy().view(np.float64)
    stat = back[168:200].copy().view(np.int32)
    key = back[200:204].copy().view(np.float32)[0]
    return _pose_fields(f[:9], f[9:18], f[18:21], stat, key)


def two_view_pose(kp1, kp2, matches, intr1, intr2, pair=(0, 1), n_hyp=DEFAULT_HYPOTHESES,
                  seed=DEFAULT_SEED, thr=DEFAULT_THRESHOLD, min_inliers=DEFAULT_MIN_INLIERS,
                  min_angle_deg=DEFAULT_MIN_ANGLE_DEG, device=0):
    """F RANSAC and the relative pose of its inliers (one upload, the F batch and the pose batch
    sfm_two_view_pose_batch, one download).  intr1 / intr2 = (f, k1, cx, cy) of the two images.

    Returns verify_pair's fields (F, inliers, count, verified, best_h) and R [3,3], t [3] (unit;
    x2 ~ R x1 + t in normalised coordinates), E [3,3] (the linear fit, unit norm), n_front (the
    inliers in front of both cameras under the winning decomposition; n_front_all the four
    candidates' counts, best the winner's index), tri_angle_deg (the median triangulation angle of
    those inliers), n_wide (how many exceed min_angle_deg) and status (0 ok, 1 fewer than
    max(min_inliers, 8) inliers, 2 degenerate; the pose fields are zero unless 0).

    The fit is linear: on a planar scene it does not recover the pose, and under pure rotation
    there is no t to recover.  Where two_view_geometry reports "planar_or_panoramic", only R and
    the angle are meaningful (R and a near-zero angle under pure rotation)."""
    import torch
    ctx, kps, pr, count, match, M, intr = _upload_pair(kp1, kp2, matches, pair, device,
                                                        intr=(intr1, intr2))
    of = ctx.ransac_batch(kps, pr, count, match, n_hyp=n_hyp, seed=seed, thr=thr,
                          min_inliers=min_inliers)
    po = ctx.two_view_pose_batch(kps, intr, pr, count, match, of["mask"], of["inl_count"],
                                 min_inliers=min_inliers, min_angle_deg=min_angle_deg)
    back = torch.cat([_pack(of, "F", M), _pack_pose(po)]).cpu().numpy()
    cnt, best_h, Fn, norm, mask = _unpack(back[:68 + M], M)
    res = dict(F=denormalize_F(Fn, norm), inliers=np.nonzero(mask)[0], count=max(cnt, 0),
               verified=cnt >= min_inliers, best_h=best_h)
    res.update(_unpack_pose(back[68 + M:68 + M + _POSE_BYTES]))
    return res


def guided_match_pair(kp1, kp2, des1, des2, pair=(0, 1), n_hyp=DEFAULT_HYPOTHESES,
                      seed=DEFAULT_SEED, thr=DEFAULT_THRESHOLD, min_inliers=DEFAULT_MIN_INLIERS,
                      guided=True, ratio=(4, 5), cross_check=sfmcore.XC_MUTUAL, max_dist=-1,
                      device=0):
    """Guided matching of one pair: match (ratio / cross_check / max_dist, as
    match_graph.GraphBuilder), verify, re-match inside the epipolar band of the estimated F
    (sfm_guided_match_batch; `guided` = True or a dict of thr, ratio, cross_check, max_dist over
    match_graph.GUIDED_DEFAULTS) and verify again with the same seed.  kp1 / kp2 [K,2] pixels,
    des1 / des2 [K,128] u8.  Equals GraphBuilder(guided=...).run on that pair.

    Returns dict(F [3,3] pixel F of the second verification, matches [M,2] (queryIdx, trainIdx)
    guided matches, dist [M] their d^2, inliers [n] indices into matches (ascending), count and
    verified of the second verification, first_count the first verification's inlier count)."""
    import torch
    from match_graph import guided_options
    gkw = guided_options(True if guided is None else guided)
    if gkw is None:
        raise ValueError("guided_match_pair: guided must be True or a dict of options")
    k1, k2 = np.asarray(kp1, np.float32).reshape(-1, 2), np.asarray(kp2, np.float32).reshape(-1, 2)
    d1, d2 = np.asarray(des1, np.uint8), np.asarray(des2, np.uint8)
    if d1.shape != (len(k1), 128) or d2.shape != (len(k2), 128):
        raise ValueError("guided_match_pair: descriptors must be [K, 128] u8, one per keypoint")
    a, b = int(pair[0]), int(pair[1])
    n_img, k_max = max(a, b) + 1, max(len(k1), len(k2), 1)
    kps = np.zeros((n_img, k_max, 2), np.float32)
    desc = np.zeros((n_img, k_max, 128), np.uint8)
    n_kp = np.zeros(n_img, np.int32)
    kps[a, :len(k1)], desc[a, :len(k1)], n_kp[a] = k1, d1, len(k1)
    kps[b, :len(k2)], desc[b, :len(k2)], n_kp[b] = k2, d2, len(k2)
    dev = torch.device("cuda", device)
    ctx = sfmcore.context(device)
    T = lambda x: torch.from_numpy(x).to(dev)
    desc_d, kps_d, n_kp_d = T(desc), T(kps), T(n_kp)
    pr = T(np.array([[a, b]], np.int32))
    rkw = dict(n_hyp=n_hyp, seed=seed, thr=thr, min_inliers=min_inliers)
    count, match, _ = ctx.match_batch(desc_d, n_kp_d, pr, metric=sfmcore.METRIC_L2,
                                      cross_check=cross_check, ratio=ratio, max_dist=max_dist)
    rs = ctx.ransac_batch(kps_d, pr, count, match, **rkw)
    gcount, gmatch, gdist = ctx.guided_match_batch(desc_d, n_kp_d, kps_d, pr, rs["inl_count"],
                                                   rs["F"], rs["norm"], min_inliers=min_inliers,
                                                   **gkw)
    rs2 = ctx.ransac_batch(kps_d, pr, gcount, gmatch, **rkw)
    M = int(gcount.item())
    cnt, _, Fn, norm, mask = _unpack(_pack(rs2, "F", M).cpu().numpy(), M)
    return dict(F=denormalize_F(Fn, norm), matches=gmatch[0, :M].cpu().numpy(),
                dist=gdist[0, :M].cpu().numpy(), inliers=np.nonzero(mask)[0], count=max(cnt, 0),
                verified=cnt >= min_inliers, first_count=max(int(rs["inl_count"].item()), 0))


def _match_array(matches) -> np.ndarray:
    if len(matches) and hasattr(matches[0], "queryIdx"):
        return np.array([[m.queryIdx, m.trainIdx] for m in matches], np.int32).reshape(-1, 2)
    return np.asarray(matches, np.int32).reshape(-1, 2)


def verify_pairs(pair_matches, keypoints, n_hyp=DEFAULT_HYPOTHESES, seed=DEFAULT_SEED,
                 thr=DEFAULT_THRESHOLD, min_inliers=DEFAULT_MIN_INLIERS, device=0,
                 chunk=8192, homography=False, h_thr=DEFAULT_H_THRESHOLD,
                 max_h_ratio=DEFAULT_MAX_H_RATIO, poses=False, intrinsics=None,
                 min_angle_deg=DEFAULT_MIN_ANGLE_DEG):
    """Verifies the reference's pair list (code/pipeline.py:36-47: Pair objects with img_inx_1,
    img_inx_2, matches; the ordered N(N-1) enumeration or any subset) in batched calls of at most
    `chunk` pairs (host and device buffers are [chunk, k_max] — constant memory however long the
    list): keypoints[i] = [K_i,2] pixel coordinates of image i.  Returns the verified
    subset (input order) with `.matches` reduced to the inliers (ascending match index) and `.F`
    (pixel F, unit norm) attached.  Results equal verify_pair on each pair (the RNG is keyed by the
    pair's image ids, so they depend neither on the batch nor on the chunking).

    homography=True: the H batch (threshold `h_thr`) runs per chunk next to the F batch on the same
    tentative matches, and every verified pair also gets `.H` (pixel H), `.h_count`, `.h_ratio` and
    `.config` (classify_two_view with `max_h_ratio`), equal to two_view_geometry on that pair.  The
    verified subset and `.matches` stay the F result.

    poses=True (with intrinsics[i] = (f, k1, cx, cy) of image i): the pose batch
    (sfm_two_view_pose_batch) runs per chunk on the F batch's masks, and every verified pair also
    gets `.R`, `.t`, `.n_front`, `.tri_angle_deg`, `.n_wide` and `.pose_status`, equal to
    two_view_pose on that pair.  Composes with homography=True; under `.config ==
    "planar_or_panoramic"` only `.R` and the angle are meaningful (a planar scene defeats the
    linear essential fit, and a pure rotation has no t)."""
    import torch
    chunk = int(chunk)
    if poses and intrinsics is None:
        raise ValueError("verify_pairs: poses=True needs intrinsics")
    if chunk < 1:   # a non-positive chunk used to return no verified pair, silently
        raise ValueError(f"verify_pairs: chunk must be >= 1, got {chunk}")
    if not pair_matches:
        return []
    pairs = np.array([[int(pr.img_inx_1), int(pr.img_inx_2)] for pr in pair_matches], np.int32)
    n_img = int(pairs.max()) + 1
    kl = [np.asarray(keypoints[i], np.float32).reshape(-1, 2) for i in range(n_img)]
    counts = np.array([len(pr.matches) for pr in pair_matches], np.int32)
    k_max = max([len(k) for k in kl] + [int(counts.max()), 1])
    kps = np.zeros((n_img, k_max, 2), np.float32)
    for i, k in enumerate(kl):
        kps[i, :len(k)] = k
    dev = torch.device("cuda", device)
    ctx = sfmcore.context(device)
    kps_d = torch.from_numpy(kps).to(dev)
    if poses:
        intr_d = torch.from_numpy(np.ascontiguousarray(
            np.asarray(intrinsics, np.float64)[:n_img].reshape(n_img, 4))).to(dev)
    verified = []
    for c0 in range(0, len(pair_matches), chunk):
        prs = pair_matches[c0:c0 + chunk]
        P = len(prs)
        match = np.zeros((P, k_max, 2), np.int32)
        for p, pr in enumerate(prs):
            m = _match_array(pr.matches)
            match[p, :len(m)] = m
        cc = counts[c0:c0 + P]
        pairs_d = torch.from_numpy(np.ascontiguousarray(pairs[c0:c0 + P])).to(dev)
        cc_d = torch.from_numpy(np.ascontiguousarray(cc)).to(dev)
        match_d = torch.from_numpy(match).to(dev)
        out = ctx.ransac_batch(kps_d, pairs_d, cc_d, match_d, n_hyp=n_hyp, seed=seed, thr=thr,
                               min_inliers=min_inliers)
        if homography:
            oh = ctx.ransac_h_batch(kps_d, pairs_d, cc_d, match_d, n_hyp=n_hyp, seed=seed,
                                    thr=h_thr, min_inliers=min_inliers)
            hcnt = oh["inl_count"].cpu().numpy()
            Hn, hnrm = oh["H"].cpu().numpy(), oh["norm"].cpu().numpy()
        if poses:
            po = ctx.two_view_pose_batch(kps_d, intr_d, pairs_d, cc_d, match_d, out["mask"],
                                         out["inl_count"], min_inliers=min_inliers,
                                         min_angle_deg=min_angle_deg)
            po = {k: v.cpu().numpy() for k, v in po.items()}
        cnt = out["inl_count"].cpu().numpy()
        mask = out["mask"].cpu().numpy()
        Fn, nrm = out["F"].cpu().numpy(), out["norm"].cpu().numpy()
        for p, pr in enumerate(prs):
            if cnt[p] >= min_inliers:
                keep = np.nonzero(mask[p, :cc[p]])[0]
                pr.matches = [pr.matches[i] for i in keep]
                pr.F = denormalize_F(Fn[p], nrm[p])
                if homography:
                    hc = max(int(hcnt[p]), 0)
                    pr.H = denormalize_H(Hn[p], hnrm[p])
                    pr.h_count = hc
                    pr.h_ratio = _h_ratio(cnt[p], hc)
                    pr.config = classify_two_view(cnt[p], hc, min_inliers, max_h_ratio)
                if poses:
                    f = _pose_fields(po["E"][p], po["R"][p], po["t"][p], po["stat"][p],
                                     po["median_key"][p])
                    pr.R, pr.t, pr.n_front = f["R"], f["t"], f["n_front"]
                    pr.tri_angle_deg, pr.n_wide = f["tri_angle_deg"], f["n_wide"]
                    pr.pose_status = f["status"]
                verified.append(pr)
    return verified
