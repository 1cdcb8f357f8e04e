"""Simulation of WHEN K2's ordered score waves learn a bound (CPU only; DESIGN.md §4.2,
profiles/k2_pilot/README.md).  Pairs of synth.make_scene(24, 4096, seed=0) (M ~ 1900, best
~ 850-970, the bench's cfg4 pairs), H = 4096, preview PV = 128, a check every 32 matches, wave-level
stops, float64 Sampson on an SVD fit (not the bit-exact f32 spec: the shares move in the third
digit).  Prints the share of (hypothesis, match) evaluations executed, preview included, under:
  seq       block bx sees the final best of all earlier blocks from its first match (the model of
            tests/perf/ransac_prune_sim.py)
  conc      ASSUMPTION: block k = 1..6 starts STAGGER * k sweeps after block 0 and sees block 0's
            bound only once block 0 has finished its full sweep; later blocks as seq.  STAGGER
            (default 0.15) is a guess at the resident window, not a measurement; the measured
            per-block table (tests/perf/ransac_wave_stops.py) shows only block 1 late.
  pilot256  block 0 of every pair first, then the rest with its bound
  running   block 0 publishes a running lower bound every period (not exact as built: rejected)
  pilot     one pilot wave (ranks 0..63 of the preview order) first, every other wave starts with
            its bound — the schedule ransac_batch runs
  ideal     the final best known from the start
Usage: NP=6 python tests/perf/ransac_pilot_sim.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "sfm-project_amd"), os.path.join(ROOT, "oracle")]

import numpy as np

import oracle as O
import synth

PV, PE, H = 128, 32, 4096
STAGGER = float(os.environ.get("STAGGER", "0.15"))
KINDS = ("seq", "conc", "pilot256", "running", "pilot", "ideal")


def masks_of(x1, x2, a, b):
    """[H, M] inlier decisions of every hypothesis (Hartley-normalised SVD fit, Sampson < 1 px^2)."""
    M = len(x1)
    c1 = x1.mean(0); s1 = np.sqrt(2) / np.mean(np.linalg.norm(x1 - c1, axis=1))
    c2 = x2.mean(0); s2 = np.sqrt(2) / np.mean(np.linalg.norm(x2 - c2, axis=1))
    X1, X2 = (x1 - c1) * s1, (x2 - c2) * s2
    h1, h2 = np.c_[X1, np.ones(M)], np.c_[X2, np.ones(M)]
    masks = np.zeros((H, M), bool)
    for h in range(H):
        idx = O.sample8(42, a, b, h, M)
        A = np.c_[X2[idx, 0:1] * X1[idx], X2[idx, 0:1], X2[idx, 1:2] * X1[idx], X2[idx, 1:2],
                  X1[idx], np.ones((8, 1))]
        F = np.linalg.svd(A)[2][-1].reshape(3, 3)
        u, sv, v = np.linalg.svd(F)
        F = u @ np.diag([sv[0], sv[1], 0]) @ v
        aa, bb = h1 @ F.T, h2 @ F
        r = np.sum(h2 * aa, 1)
        e = s2 * s2 * (aa[:, 0] ** 2 + aa[:, 1] ** 2) + s1 * s1 * (bb[:, 0] ** 2 + bb[:, 1] ** 2) - r * r
        masks[h] = e > 0
    return masks


def shares(masks):
    M = masks.shape[1]
    cnt, cum = masks.sum(1), np.cumsum(masks, 1)
    chk = np.arange(PV + PE, M + PE, PE).clip(max=M)
    order = np.argsort(-cum[:, PV - 1], kind="stable")
    L = M - PV
    fin = [cnt[order[bx * 256:(bx + 1) * 256]].max() for bx in range(H // 256)]
    pilot = cnt[order[:64]].max()
    b0 = order[:256]

    def wave_work(lanes, bound_at):   # bound_at(matches scored past the preview) -> bound
        for m in chk:
            if np.all(cum[lanes, m - 1] + (M - m) < bound_at(m - PV)):
                return m - PV
        return L

    out = []
    for kind in KINDS:
        work = 0
        for bx in range(H // 256):
            prevb = max(fin[:bx]) if bx else 0
            for w in range(4):
                lanes = order[bx * 256 + w * 64:bx * 256 + (w + 1) * 64]
                if kind == "seq":
                    f = lambda d: prevb
                elif kind == "conc":
                    arrive = max(0.0, 1 - STAGGER * bx) * L
                    f = ((lambda d: 0) if bx == 0 else
                         (lambda d: fin[0] if d >= arrive else 0) if bx < 7 else (lambda d: prevb))
                elif kind == "pilot256":
                    f = (lambda d: 0) if bx == 0 else (lambda d: fin[0])
                elif kind == "running":
                    f = ((lambda d: int(cum[b0, min(M, PV + d) - 1].max())) if bx == 0 else
                         (lambda d: int(cum[b0, min(M, PV + int(d + STAGGER * bx * L)) - 1].max()))
                         if bx < 7 else (lambda d: prevb))
                elif kind == "pilot":
                    f = (lambda d: 0) if bx == 0 and w == 0 else (lambda d: pilot)
                else:
                    f = lambda d: cnt.max()
                work += 64 * wave_work(lanes, f)
        out.append(work + H * PV)
    return np.array(out, np.float64), H * M


def main():
    n_img = int(os.environ.get("NI", "24"))
    s = synth.make_scene(n_img, 4096, seed=0)
    pairs = synth.unordered_pairs(n_img)
    rng = np.random.default_rng(1)
    tot, full = np.zeros(len(KINDS)), 0
    for p in rng.choice(len(pairs), int(os.environ.get("NP", "6")), replace=False):
        a, b = (int(x) for x in pairs[p])
        q, t, _ = O.match(s["desc"][a], s["desc"][b], 0, 1, (4, 5))
        if len(q) < 300:
            continue
        m = masks_of(s["kps"][a][q].astype(np.float64), s["kps"][b][t].astype(np.float64), a, b)
        r, f = shares(m)
        tot += r
        full += f
        print(p, "M", len(q), "best", int(m.sum(1).max()),
              {k: round(float(v), 3) for k, v in zip(KINDS, r / f)}, flush=True)
    sc = tot / full
    print("share executed, preview included:", {k: round(float(v), 3) for k, v in zip(KINDS, sc)})


if __name__ == "__main__":
    main()
