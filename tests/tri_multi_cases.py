"""Seeded cases of the recursive robust triangulation tests, shared by the CPU and the GPU file
(TEST INFRASTRUCTURE ONLY).  Problems are the dicts of tests/tri_cases.py plus what was planted:
group [n_obs] i8 (the scene point of the track an observation belongs to, -1 = belongs to none
that can be recovered), truth (per track the list of its recoverable points, largest group first)
and n_points [n_pt] (how many of them the call must return)."""
from __future__ import annotations

import numpy as np

import synth
import tri_cases

SEP = 1.3          # smallest distance between two points of one merged track
BASELINE = 2.0     # smallest extent of a set's camera centres (the cameras sit at radius 8)


def _points(rng, k):
    """k points of [-2, 2]^3, pairwise at least SEP apart."""
    while True:
        X = rng.uniform(-2.0, 2.0, size=(k, 3))
        d = [np.linalg.norm(X[i] - X[j]) for i in range(k) for j in range(i + 1, k)]
        if not d or min(d) >= SEP:
            return X


def merged(rng, cams, sizes, lost=(), shuffle=True):
    """A track merged out of len(sizes) points seen from disjoint camera sets, 0.25 px noise
    (a two-view point from a narrow pair then stays within 0.1 of the truth).
    Groups listed in `lost` are planted but cannot be recovered (their observations count as
    -1).  Returns (track tuple of tri_cases._problem, group per observation, truths)."""
    X = _points(rng, len(sizes))
    centres = synth.camera_centres(cams)
    ends = np.cumsum(sizes)
    while True:
        # the two widest cameras of every set at least BASELINE apart: a two- or three-view set
        # then passes the angle gate and fixes its depth to well within 0.1
        cl = rng.choice(len(cams), size=int(sum(sizes)), replace=False)
        sets = [centres[cl[e - n:e]] for n, e in zip(sizes, ends)]
        if all(len(c) < 2 or np.linalg.norm(c[:, None] - c[None], axis=2).max() >= BASELINE
               for c in sets):
            break
    cam_list, uv, group = [], [], []
    at = 0
    for g, n in enumerate(sizes):
        t = tri_cases._track(rng, cams, cl[at:at + n], X[g], noise=0.25)
        at += n
        cam_list += [int(c) for c in t[0]]
        uv.append(t[1])
        group += [-1 if g in lost else g] * n
    uv = np.concatenate(uv)
    order = rng.permutation(len(cam_list)) if shuffle else np.arange(len(cam_list))
    track = ([cam_list[i] for i in order], uv[order], None, None)
    return track, [group[i] for i in order], [X[g] for g in range(len(sizes)) if g not in lost]


def _assemble(cams, pp, items, ids=None):
    """items: (track, group, truths) of merged() or None for an empty track."""
    empty = ([], np.zeros((0, 2)), None, None)
    prob = tri_cases._problem(cams, pp, [it[0] if it else empty for it in items], ids=ids)
    prob["group"] = np.array([g for it in items if it for g in it[1]], np.int8).reshape(-1)
    prob["truth"] = [it[2] if it else [] for it in items]
    prob["n_points"] = np.array([len(it[2]) if it else 0 for it in items], np.int32)
    return prob


def _single(rng, cams):
    """A one-observation track: nothing to recover."""
    t, g, _ = merged(rng, cams, [1])
    return t, [-1], []


def merges(seed=4):
    """List of (name, problem, keyword arguments of the call).  Under some seeds a pixel of one
    set happens to lie within the threshold of another set's point; tests/
    test_triangulate_multi_cpu.py checks that this one plants what it says."""
    rng = np.random.Generator(np.random.PCG64([seed, 0x7A3]))
    # azimuth within +-35 degrees: two rays to a point never meet at more than 90 degrees, which
    # the two-view step rejects (c > 0), so a two-observation set always has its hypothesis
    cams, pp = tri_cases._cameras(rng, 520, 35.0, 20.0)
    out = []
    M = lambda *sizes, **kw: merged(rng, cams, list(sizes), **kw)

    def miss():
        # 5 + 2, the last two rays missing each other by 120 px (cameras differ mostly in
        # azimuth: off the epipolar line): round 1 has no admissible hypothesis
        t, g, X = M(5, 2, lost=(1,), shuffle=False)
        t[1][6] += np.array([0.0, 120.0])
        return t, g, X

    # round 0 + later rounds across every list boundary: short lists (<= 8, <= 16, <= 32
    # hypotheses), the long list (> 16 observations or > 32 hypotheses), sampled against
    # enumerated pairs at max_hyp 64, the 128-record staging
    main = [M(2, 2), None, M(3, 2), M(4, 4), _single(rng, cams), M(9, 8), M(12, 11), None, None,
            M(70, 66), M(129, 5), M(6, 5, 4), M(5, 1, lost=(1,)), miss(), _single(rng, cams)]
    prob = _assemble(cams, pp, main)
    out.append(("merges", prob, dict(max_points=3)))
    out.append(("merges_seed_wraps", prob, dict(max_points=3, seed=2 ** 64 - 1)))
    out.append(("min_views_3", _assemble(cams, pp, [M(5, 2, lost=(1,)), M(5, 3)], ids=[4, 11]),
                dict(max_points=3, min_views=3)))
    out.append(("max_points_2", _assemble(cams, pp, [M(6, 5, 4, lost=(2,)), M(3, 2)], ids=[2, 5]),
                dict(max_points=2)))
    out.append(("n_pt_0", _assemble(cams, pp, []), dict(max_points=3)))
    out.append(("n_pt_1", _assemble(cams, pp, [M(3, 2)], ids=[77]), dict(max_points=3)))
    # more than one block of tracks; sets of >= 3, so that a pair of rays of two different points
    # that happen to pass each other (a phantom consensus of 2) never ties with a planted set
    many = []
    for _ in range(257):
        k = int(rng.integers(1, 4))
        many.append(M(*[int(v) for v in sorted(rng.integers(3, 7, size=k))[::-1]]))
    out.append(("n_pt_257", _assemble(cams, pp, many), dict(max_points=3)))
    return out


def no_later_round(seed=4):
    """A batch in which every track ends in round 0: empty and one-observation tracks (status 1)
    and two-observation tracks whose rays miss each other (status 4)."""
    rng = np.random.Generator(np.random.PCG64([seed, 0x7A4]))
    cams, pp = tri_cases._cameras(rng, 64, 35.0, 0.5)   # baselines along u: 120 px in v miss
    items = []
    for i in range(300):
        if i % 3 == 0:
            items.append(None)
        elif i % 3 == 1:
            items.append(_single(rng, cams))
        else:
            t, g, _ = merged(rng, cams, [2], lost=(0,), shuffle=False)
            t[1][1] += np.array([0.0, 120.0])
            items.append((t, g, []))
    return _assemble(cams, pp, items)
