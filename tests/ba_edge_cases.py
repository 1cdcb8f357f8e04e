"""Seeded cases for the bundle-adjustment linearisation (sfm_ba_jtj / sfm_ba_cost, csrc/ba.hip),
shared by the CPU test (test_ba_hp_cpu.py) and the GPU test (test_gpu_ba_hp.py); numpy +
tests/hp_ref.py.  Cases and their references are built once per process.

case(name) -> dict cams [n_cam,8], pp [n_cam,2], pts [n_pt,3], cam_idx, pt_idx (point-major), uv,
and for "edge" regime [n_obs] / value [n_obs]: the regime an observation belongs to and its
setting.  reference(name, loss_s) -> (ref, unit): float64 dicts over hp_ref.BA_OUTPUTS.

  "edge"  416 observations, each in one regime, everything else benign (|r| 0.1-0.5, depth ~8,
          |k1| <= 0.02, 0.5 px noise, f ~1000); reference: hp_ref.ba_assemble (50 digits, Jacobian
          by central differences), at every loss_s of EDGE_LOSS = (0, 1e-3, 2, 1e6)
    rotation    |r| in ROT_NORMS = 0, 1e-11, 2e-10 (both sides of |r|^2 = 1e-20), 5e-7, 1e-6, 1e-3,
                0.3, 1, 2.5, pi - 1e-3, pi - 1e-8; axes e_x, e_y, e_z and five random ones; two
                observations per camera, two per point.  (5e-7 is there for mutation e: at 2e-10 a
                first-order rotation is exact in float64, at 1e-6 |r|^2 sits on the mutated switch)
    depth       P2 in 0.05, 0.5, 8, 1e3, 1e5 with |t|, |X| ~ max(8, depth); own camera and point
    distortion  k1 in -0.3, -0.05, 0, 0.05, 0.3, |p| from 0.1 to 0.9 (1 + k1 |p|^2 >= 0.5)
    loss        residuals of 1e-9, 0.5, 40, 1e4 and 1e-6 px: with EDGE_LOSS the pairs (1e-9, 1e-3),
                (0.5, 2), (40, 2), (1e4, 1e-3), (1e-6, 1e6) and every other combination
    isolated    cameras and points with exactly one observation each
    benign      6 cameras x 24 points, 3 views each
          plus a camera without observations and points without at both ends and in the middle.
  "S1"    6 cameras holding 0, 1, 15, 16, 17, 300 observations (16 splits per camera and
          ba_final_kernel: empty splits, splits starting past the camera's end); loss_s = 2
  "S2a"   260 cameras (one wave per camera): the first nine hold 0, 1, 63, 64, 65, 127, 128, 129,
          257 observations (the camera wave's stride is CAM_MLP 64 = 128), the rest 1-3; tracks of
          0, 1, 2, 63, 64, 65, 150, 257: the 150-track starts at lane 1 of a wave, the 257-track at
          lane 63 and ends on a wave's last lane, the 64-track ends on the last lane of a
          256-block; points without observations at both ends; n_obs = 1536 = 6 x 256
  "S2b"   the same with n_obs = 1499 (no multiple of 64)
          Shape cases: benign parameters; reference = 50-digit residual, rho and cost, Jacobians
          from the float64 restatement (hp_ref.ba_f64), sums by math.fsum.

Tolerance.  Every entry q of every output has a unit u(q) (hp_ref.ba_units): the first-order
propagation of a relative eps on t, X, f, k1, pp, uv and an absolute eps on the entries of R
through the linearisation, with u(ab) = |a|u(b) + |b|u(a) + eps|ab| and u(sum) = sum u +
eps sum|term|.  An entry whose unit is 0 must match exactly; a NaN or an infinity fails.
K = 4 x the worst ratio |oracle - reference| / unit of the CPU oracle (oracle/sfm_oracle_ba.c)
over all cases and outputs; the factor 4 is for the kernel's summation order and its sincos.

Measured (test_ba_hp_cpu.py prints them), worst ratio of the CPU oracle:
  per case    edge 0.424 at every loss_s (the residual of a 1e4 px observation), S1 0.132,
              S2a 0.187, S2b 0.187                                          (ORACLE_RATIO)
  per output  res 0.424, W 0.236, U 0.210, V 0.158, gc 0.134, gp 0.173, cost 0.088
  per regime  (res / W at loss_s 0) flat: 0.04-0.13 / 0.06-0.24 in every regime but the 1e4 px
              residuals (0.42 / 0.15); next to pi 0.13 / 0.20, |r| <= 2e-10 0.10 / 0.13,
              depth 0.05 0.13 / 0.12, depth 1e5 0.08 / 0.09
  oracle_ba_obs alone: J 0.308, rho 0.291
hence K = 4 x 0.424 = 1.696.  Each of the eight mutations of the restatement (a wrong cross term,
a flipped sign in -[Y]x, d/dk1 without f, e/s for e/s^2, the first-order rotation up to 1e-12,
float32 sin / cos, one observation dropped from a 129-observation camera, log for log1p) lands
176 to 1e19 times outside K.
Measured on an MI355X (test_gpu_ba_hp.py prints them per case, output and mode), the kernel's
worst ratio over the plain, chunked (8, 3) and export forms:
  per case    edge 0.424 at every loss_s, S1 0.132, S2a 0.187, S2b 0.187
  per output  res 0.424, W 0.207, U 0.210, V 0.158, gc 0.134, gp 0.173, cost 0.176
  sfm_ba_cost against the reference <= 0.176; against the linearisation's cost 0 summation units
  (the same bits) in every case and mode
Nothing was found: the kernel sits where the oracle does, a quarter of K.
"""
from __future__ import annotations

import functools

import numpy as np

import hp_ref

EPS = hp_ref.EPS
PP = (960.0, 540.0)
EDGE_LOSS = (0.0, 1e-3, 2.0, 1e6)
SHAPE_LOSS = 2.0
ROT_NORMS = (0.0, 1e-11, 2e-10, 5e-7, 1e-6, 1e-3, 0.3, 1.0, 2.5, np.pi - 1e-3, np.pi - 1e-8)
DEPTHS = (0.05, 0.5, 8.0, 1e3, 1e5)
K1S = (-0.3, -0.05, 0.0, 0.05, 0.3)
RESIDUALS = (1e-9, 0.5, 40.0, 1e4, 1e-6)
S1_COUNTS = (0, 1, 15, 16, 17, 300)
S2_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 257)
S2_TRACKS = (0, 1, 2, 63, 64, 65, 150, 257)
S2_NOBS = dict(S2a=1536, S2b=1499)
CASES = tuple(("edge", s) for s in EDGE_LOSS) + tuple((n, SHAPE_LOSS) for n in ("S1", "S2a", "S2b"))

# worst |oracle - reference| / unit of the CPU oracle per (case, loss_s), measured
ORACLE_RATIO = {
    ("edge", 0.0): 0.424, ("edge", 1e-3): 0.424, ("edge", 2.0): 0.424, ("edge", 1e6): 0.424,
    ("S1", 2.0): 0.132, ("S2a", 2.0): 0.187, ("S2b", 2.0): 0.187,
}
K = 4 * max(ORACLE_RATIO.values())      # 1.696


def case_id(c):
    return f"{c[0]}@{c[1]:g}"


def _unit(rng):
    d = rng.normal(size=3)
    return d / np.linalg.norm(d)


def _R(r):
    return hp_ref.rotmat_f64(r)[0]


def _project(cam, pp, X):
    P = _R(cam[:3]) @ X + cam[3:6]
    q = P[:2] / P[2]
    return cam[6] * (1.0 + cam[7] * (q @ q)) * q + pp


def _benign_cam(rng, r=None, k1=None):
    """A camera ~8 in front of the unit box looking along +z: any rotation r keeps the box in
    front of it, since t alone sets the depth."""
    cam = np.zeros(8)
    cam[:3] = rng.uniform(0.1, 0.5) * _unit(rng) if r is None else r
    cam[3:6] = (rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(7.5, 8.5))
    cam[6] = rng.uniform(950.0, 1050.0)
    cam[7] = rng.uniform(-0.02, 0.02) if k1 is None else k1
    return cam


class _Builder:
    def __init__(self, rng):
        self.rng, self.cams, self.pp, self.pts, self.obs = rng, [], [], [], []

    def cam(self, cam):
        self.cams.append(cam)
        self.pp.append(np.array(PP) + self.rng.uniform(-5, 5, size=2))
        return len(self.cams) - 1

    def pt(self, X):
        self.pts.append(np.asarray(X, np.float64))
        return len(self.pts) - 1

    def at(self, c, Pc):
        """The world point that camera c sees at camera-frame position Pc."""
        cam = self.cams[c]
        return self.pt(np.linalg.solve(_R(cam[:3]), np.asarray(Pc) - cam[3:6]))

    def see(self, c, p, regime, value, residual=None):
        uv = _project(self.cams[c], self.pp[c], self.pts[p])
        if residual is None:
            uv = uv + self.rng.normal(0.0, 0.5, size=2)
        else:
            a = self.rng.uniform(0, 2 * np.pi)
            uv = uv + residual * np.array([np.cos(a), np.sin(a)])
        self.obs.append((p, c, uv[0], uv[1], regime, value))

    def problem(self):
        order = sorted(range(len(self.obs)), key=lambda i: self.obs[i][0])
        o = [self.obs[i] for i in order]
        return dict(cams=np.array(self.cams), pp=np.array(self.pp), pts=np.array(self.pts),
                    cam_idx=np.array([x[1] for x in o], np.int32),
                    pt_idx=np.array([x[0] for x in o], np.int32),
                    uv=np.array([[x[2], x[3]] for x in o]),
                    regime=np.array([x[4] for x in o]), value=np.array([x[5] for x in o]))


def _front(rng, spread=0.2):
    z = rng.uniform(7.0, 9.0)
    return np.array([rng.uniform(-spread, spread) * z, rng.uniform(-spread, spread) * z, z])


def _edge(seed=11):
    rng = np.random.default_rng(seed)
    b = _Builder(rng)
    b.pt(rng.uniform(-1, 1, size=3))                                  # unobserved, first
    axes = [np.eye(3)[i] for i in range(3)] + [_unit(rng) for _ in range(5)]
    for rn in ROT_NORMS:                                              # rotation
        cs = [b.cam(_benign_cam(rng, r=rn * a)) for a in axes]
        ps = [b.at(c, _front(rng)) for c in cs]
        for i, c in enumerate(cs):
            b.see(c, ps[i], "rotation", rn)
            b.see(c, ps[(i + 1) % len(cs)], "rotation", rn)
    for dep in DEPTHS:                                                # depth
        for _ in range(8):
            cam = _benign_cam(rng)
            X = max(8.0, dep) * rng.uniform(0.5, 1.5) * _unit(rng)
            Pc = dep * np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0])
            cam[3:6] = Pc - _R(cam[:3]) @ X
            b.see(b.cam(cam), b.pt(X), "depth", dep)
    b.pt(rng.uniform(-1, 1, size=3))                                  # unobserved, middle
    for k1 in K1S:                                                    # distortion
        c = b.cam(_benign_cam(rng, k1=k1))
        for pn in np.linspace(0.1, 0.9, 8):
            a, z = rng.uniform(0, 2 * np.pi), rng.uniform(7.0, 9.0)
            b.see(c, b.at(c, z * np.array([pn * np.cos(a), pn * np.sin(a), 1.0])), "distortion", k1)
    cs = [b.cam(_benign_cam(rng)) for _ in range(4)]                  # loss
    for rs in RESIDUALS:
        for i in range(8):
            p = b.pt(rng.uniform(-1, 1, size=3))
            for c in (cs[i % 4], cs[(i + 1 + i // 4) % 4]):
                b.see(c, p, "loss", rs, residual=rs)
    for _ in range(8):                                                # isolated
        c = b.cam(_benign_cam(rng))
        b.see(c, b.at(c, _front(rng)), "isolated", 1.0)
    cs = [b.cam(_benign_cam(rng)) for _ in range(6)]                  # benign
    for i in range(24):
        p = b.pt(rng.uniform(-1, 1, size=3))
        for c in rng.choice(6, size=3, replace=False):
            b.see(cs[c], p, "benign", 0.0)
    b.cam(_benign_cam(rng))                                           # unobserved camera
    b.pt(rng.uniform(-1, 1, size=3))                                  # unobserved, last
    return b.problem()


def _assign(rng, cam_counts, lengths):
    """Cameras for every track (distinct within a track) such that camera c gets exactly
    cam_counts[c] observations: longest track first, each to the cameras with the most left."""
    left = np.array(cam_counts, np.int64)
    assert left.sum() == sum(lengths)
    tracks = [None] * len(lengths)
    for t in sorted(range(len(lengths)), key=lambda i: -lengths[i]):
        L = lengths[t]
        pick = np.lexsort((rng.random(len(left)), -left))[:L]
        assert L == 0 or left[pick].min() > 0, "track lengths do not fit the camera counts"
        left[pick] -= 1
        tracks[t] = rng.permutation(pick).tolist()
    assert not left.any()
    return tracks


def _shape_problem(rng, cam_counts, lengths):
    n_cam = len(cam_counts)
    cams = np.array([_benign_cam(rng) for _ in range(n_cam)])
    cams[:, 7] = rng.uniform(-0.05, 0.05, size=n_cam)
    pp = np.tile(PP, (n_cam, 1)) + rng.uniform(-5, 5, size=(n_cam, 2))
    pts = rng.uniform(-1, 1, size=(len(lengths), 3))
    ci, pi, uv = [], [], []
    for p, cs in enumerate(_assign(rng, cam_counts, lengths)):
        for c in cs:
            ci.append(c)
            pi.append(p)
            uv.append(_project(cams[c], pp[c], pts[p]) + rng.normal(0.0, 0.5, size=2))
    return dict(cams=cams, pp=pp, pts=pts, cam_idx=np.array(ci, np.int32),
                pt_idx=np.array(pi, np.int32), uv=np.array(uv))


def _s1(seed=12):
    rng = np.random.default_rng(seed)
    mid = [5] + [4] * 4 + [3] * 7 + [2] * 8 + [0] * 3
    mid += [1] * (sum(S1_COUNTS) - sum(mid))
    return _shape_problem(rng, S1_COUNTS, [0] + rng.permutation(mid).tolist() + [0])


def _fill(rng, total):
    """Track lengths 1-2 (and a few 0) summing to total."""
    out = []
    while total > 0:
        L = min(total, int(rng.integers(1, 3)))
        out.append(L)
        total -= L
        if rng.random() < 0.03:
            out.append(0)
    return out


def _s2(name):
    rng = np.random.default_rng(dict(S2a=13, S2b=14)[name])
    n_obs = S2_NOBS[name]
    rest = np.ones(260 - len(S2_COUNTS), np.int64)
    extra = n_obs - sum(S2_COUNTS) - len(rest)
    assert 0 <= extra <= 2 * len(rest)
    while extra:
        i = rng.integers(len(rest))
        if rest[i] < 3:
            rest[i] += 1
            extra -= 1
    # observation index:  0 | 1..150 | 151..190 | 191..447 | 448..511 | 512..576 | 577..639 | ...
    head = [0, 1, 150] + [2] * 20 + [257, 64, 0, 65, 63, 2]
    lengths = head + _fill(rng, n_obs - sum(head)) + [0]
    return _shape_problem(rng, list(S2_COUNTS) + rest.tolist(), lengths)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _edge() if name == "edge" else _s1() if name == "S1" else _s2(name)
    for v in c.values():
        v.setflags(write=False)
    return c


def _args(c):
    return c["cams"], c["pp"], c["pts"], c["cam_idx"], c["pt_idx"], c["uv"]


@functools.lru_cache(maxsize=None)
def reference(name, loss_s):
    """(ref, unit) of a case at loss_s; ref also holds J, w, rho per observation."""
    c = case(name)
    if name == "edge":
        ref = hp_ref.ba_assemble(*_args(c), loss_s)
        unit = ref.pop("unit")
    else:
        ref, unit = hp_ref.ba_f64(*_args(c), loss_s, exact=True)
        ref["res"], ref["rho"], ref["cost"] = hp_ref.ba_residuals(*_args(c), loss_s)
    for d in (ref, unit):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return ref, unit


def ratios(name, loss_s, out, keys=hp_ref.BA_OUTPUTS):
    """Worst |out - reference| / unit per output.  An entry with unit 0 must match exactly, and a
    NaN or an infinity counts as infinitely far."""
    ref, unit = reference(name, loss_s)
    worst = {}
    for k in keys:
        a = np.asarray(out[k], np.float64).reshape(np.shape(ref[k]))
        u = np.asarray(unit[k], np.float64)
        d = np.abs(a - ref[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(u > 0, d / u, np.where(d == 0, 0.0, np.inf))
        q = np.where(np.isfinite(a), q, np.inf)
        worst[k] = float(q.max()) if q.size else 0.0
    return worst


def check(name, loss_s, out, label, k=None):
    """Prints and asserts the ratios of one linearisation against K."""
    k = K if k is None else k
    r = ratios(name, loss_s, out)
    print(f"{name}@{loss_s:g} {label}: " + " ".join(f"{o}={v:.3f}" for o, v in r.items())
          + f"  (allowed {k:.2f})")
    bad = {o: v for o, v in r.items() if not v <= k}
    assert not bad, f"{name}@{loss_s:g} {label}: outside {k:.3g} units: {bad}"
    return r
