"""Seeded cases of the robust triangulation tests, shared by the CPU and the GPU file (TEST
INFRASTRUCTURE ONLY).  A problem is a dict of host arrays: cams [n_cam,8], pp [n_cam,2], pt_ptr
[n_pt+1] i32, cam_idx [n_obs] i32, uv [n_obs,2] f64, pt_id [n_pt] i32, and where they are known
pts [n_pt,3] (the truth) and planted [n_obs] u8 (1 = a true observation)."""
from __future__ import annotations

import numpy as np

import synth

CX, CY = synth.WIDTH / 2.0, synth.HEIGHT / 2.0


def _cameras(rng, n_cam, az_deg, el_deg, k1_range=0.02, radius=8.0):
    """Cameras on the scene's sphere, azimuth / elevation uniform in +-az_deg / +-el_deg, looking
    at the origin."""
    cams = np.zeros((n_cam, 8))
    for i in range(n_cam):
        az = np.deg2rad(rng.uniform(-az_deg, az_deg))
        el = np.deg2rad(rng.uniform(-el_deg, el_deg))
        C = radius * np.array([np.sin(az) * np.cos(el), np.sin(el), np.cos(az) * np.cos(el)])
        R = synth._look_at(C)
        cams[i, :3] = synth.rotmat_to_angle_axis(R)
        cams[i, 3:6] = -R @ C
        cams[i, 6] = synth.FOCAL
        cams[i, 7] = rng.uniform(-k1_range, k1_range)
    return cams, np.tile(np.array([CX, CY]), (n_cam, 1))


def _project(cam, X):
    R = synth.angle_axis_to_rotmat(cam[:3])
    uv, z = synth.project(R, cam[3:6], cam[6], cam[7], CX, CY, np.asarray(X, np.float64)[None])
    return uv[0], z[0]


def _problem(cams, pp, tracks, ids=None):
    """tracks: list of (cam list, uv [n,2], truth or None, planted list or None)."""
    ptr = np.r_[0, np.cumsum([len(t[0]) for t in tracks])].astype(np.int32)
    cam_idx = np.array([c for t in tracks for c in t[0]], np.int32).reshape(-1)
    uv = (np.concatenate([np.asarray(t[1], np.float64).reshape(-1, 2) for t in tracks])
          if tracks else np.zeros((0, 2)))
    pts = np.array([t[2] if t[2] is not None else np.zeros(3) for t in tracks]).reshape(-1, 3)
    planted = np.array([m for t in tracks for m in (t[3] if t[3] is not None
                                                    else [1] * len(t[0]))], np.uint8).reshape(-1)
    pt_id = np.arange(len(tracks), dtype=np.int32) if ids is None else np.asarray(ids, np.int32)
    return dict(cams=cams, pp=pp, pt_ptr=ptr, cam_idx=cam_idx, uv=uv, pts=pts, planted=planted,
                pt_id=pt_id)


def _track(rng, cams, cam_list, X, noise=0.5, n_out=0):
    """Observations of X in cam_list with Gaussian noise; n_out of them displaced by 50 .. 400 px
    in a random direction."""
    uv = np.array([_project(cams[c], X)[0] for c in cam_list]).reshape(-1, 2)
    uv = uv + rng.normal(0.0, noise, size=uv.shape)
    planted = np.ones(len(cam_list), np.uint8)
    if n_out:
        bad = rng.choice(len(cam_list), size=n_out, replace=False)
        ang = rng.uniform(0.0, 2.0 * np.pi, size=n_out)
        uv[bad] += rng.uniform(50.0, 400.0, size=n_out)[:, None] * np.stack([np.cos(ang),
                                                                             np.sin(ang)], 1)
        planted[bad] = 0
    return list(cam_list), uv, np.asarray(X, np.float64), planted


def planted_outliers(seed=0, n_tracks=3000, n_cam=64):
    """(a): tracks of 4 .. 13 views of a point uniform in [-2, 2]^3 from cameras at azimuth
    +-15 / elevation +-10 degrees, 0.5 px noise, up to (n - 1) // 3 planted outliers."""
    rng = np.random.Generator(np.random.PCG64([seed, 0x7A1]))
    cams, pp = _cameras(rng, n_cam, 15.0, 10.0)
    tracks = []
    for _ in range(n_tracks):
        n = int(rng.integers(4, 14))
        cl = rng.choice(n_cam, size=n, replace=False)
        X = rng.uniform(-2.0, 2.0, size=3)
        tracks.append(_track(rng, cams, cl, X, n_out=int(rng.integers(0, (n - 1) // 3 + 1))))
    return _problem(cams, pp, tracks)


def reorder(prob, order):
    """The tracks `order` of prob (a permutation or a subset), pt_id kept."""
    order = np.asarray(order, np.int64)
    ptr = prob["pt_ptr"]
    obs = (np.concatenate([np.arange(ptr[t], ptr[t + 1]) for t in order])
           if len(order) else np.zeros(0, np.int64)).astype(np.int64)
    out = dict(prob)
    out["pt_ptr"] = np.r_[0, np.cumsum(ptr[order + 1] - ptr[order])].astype(np.int32)
    for k in ("cam_idx", "uv", "planted"):
        out[k] = prob[k][obs]
    for k in ("pts", "pt_id"):
        out[k] = prob[k][order]
    out["obs"] = obs      # where each observation was in prob
    return out


def edge_cases(seed=1):
    """(b): list of (name, problem, keyword arguments of the call)."""
    rng = np.random.Generator(np.random.PCG64([seed, 0x7A2]))
    cams, pp = _cameras(rng, 520, 60.0, 20.0)
    out = []
    P = lambda: rng.uniform(-2.0, 2.0, size=3)

    def plain(n, frac_out=0.0):
        cl = rng.choice(len(cams), size=n, replace=False)
        return _track(rng, cams, cl, P(), n_out=int(frac_out * n))

    empty = ([], np.zeros((0, 2)), None, None)
    # track lengths: below 2, the exhaustive / sampled switch (55 and 66 pairs against 64), the
    # 16 / 17 switch to the long-track bin, that bin's staging capacity (128 records) and beyond,
    # empty tracks in the middle
    lens = [0, 1, 2, 3, 11, 12, 0, 0, 64, 65, 5, 257, 0, 513, 4, 0, 16, 17, 128, 129]
    out.append(("lengths", _problem(cams, pp, [plain(n, 0.1 if n > 12 else 0.0) if n else empty
                                               for n in lens]), {}))
    # max_hyp around the wave size on one 40-view track (780 pairs: sampled everywhere)
    t40 = plain(40, 0.2)
    for mh in (1, 63, 64, 65, 256):
        out.append((f"max_hyp_{mh}", _problem(cams, pp, [t40], ids=[7]), dict(max_hyp=mh)))
    # few hypotheses on a 12-view track: more observations than the short bins stage (4 / 6 / 8)
    t12 = plain(12, 0.1)
    for mh in (4, 12, 24):
        out.append((f"max_hyp_{mh}_of_12_views", _problem(cams, pp, [t12, plain(3)], ids=[3, 9]),
                    dict(max_hyp=mh)))
    # a camera twice in a track (its pair has no baseline)
    t = plain(4)
    t = ([t[0][0]] + t[0], np.concatenate([t[1][:1] + 0.25, t[1]]), t[2], None)
    out.append(("repeated_camera", _problem(cams, pp, [t, plain(5)]), {}))
    # every pair narrower than the angle gate: status 4
    ncams, npp = _cameras(rng, 6, 0.2, 0.2)
    tn = _track(rng, ncams, list(range(6)), P())
    out.append(("narrow", _problem(ncams, npp, [tn, tn]), dict(min_angle_deg=2.0)))
    # a point behind one camera: that camera looks away from the scene
    bc = cams.copy()
    Rb = synth.angle_axis_to_rotmat(bc[0, :3])
    Cb = -Rb.T @ bc[0, 3:6]
    Rf = np.diag([-1.0, 1.0, -1.0]) @ Rb          # turned by 180 degrees about its y axis
    bc[0, :3] = synth.rotmat_to_angle_axis(Rf)
    bc[0, 3:6] = -Rf @ Cb
    X = P()
    tb = _track(rng, bc, [0, 1, 2, 3, 4], X)
    assert _project(bc[0], X)[1] < 0
    tb[3][0] = 0
    out.append(("behind", _problem(bc, pp, [tb]), {}))
    # two-observation tracks whose rays miss each other by far more than thr: status 4
    miss = []
    for _ in range(4):
        t = plain(2)
        t[1][1] += np.array([0.0, 120.0])   # cameras differ mostly in azimuth: off the epipolar line
        miss.append((t[0], t[1], t[2], [0, 0]))
    out.append(("two_view_miss", _problem(cams, pp, miss + [plain(2)]), {}))
    # batch sizes
    out.append(("n_pt_0", _problem(cams, pp, []), {}))
    out.append(("n_pt_1", _problem(cams, pp, [plain(5)]), {}))
    out.append(("n_pt_257", _problem(cams, pp, [plain(int(rng.integers(2, 8))) for _ in range(257)]),
                {}))
    return out
