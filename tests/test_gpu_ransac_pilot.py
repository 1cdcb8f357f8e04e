"""K2's pilot launch (ransac.hip ransac_score_kernel; SFM_RANSAC_PILOT) and the
bound read one period ahead only change WHEN a wave learns a bound, never the result: every test
compares the full outputs (inl_count, best_h, mask[:M], F, norm) bit for bit, between the pilot
settings and against the CPU oracle."""
import os

import numpy as np
import pytest

import oracle as O
import synth

pytestmark = pytest.mark.gpu

KEYS = ("inl_count", "best_h", "F", "norm")


class _pilot:
    """SFM_RANSAC_PILOT = value (None: unset, the default) inside the block; restored after."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("SFM_RANSAC_PILOT")
        if self.value is None:
            os.environ.pop("SFM_RANSAC_PILOT", None)
        else:
            os.environ["SFM_RANSAC_PILOT"] = str(self.value)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("SFM_RANSAC_PILOT", None)
        else:
            os.environ["SFM_RANSAC_PILOT"] = self.old


def _T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _batch(ctx, kps, pairs, count, match, H, seed=42):
    import torch
    out = ctx.ransac_batch(_T(kps), _T(np.asarray(pairs, np.int32)), _T(np.asarray(count, np.int32)),
                           _T(match), n_hyp=H, seed=seed, thr=1.0)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(a, b, count):
    for k in KEYS:
        np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8), err_msg=k)
    for p, M in enumerate(count):
        np.testing.assert_array_equal(a["mask"][p, :M], b["mask"][p, :M], err_msg=f"mask {p}")


def _vs_oracle(out, p, r, M, f64=False):
    u = np.uint64 if f64 else np.uint32
    assert out["inl_count"][p] == r["count"] and out["best_h"][p] == r["best_h"], f"pair {p}"
    if M >= 8:
        np.testing.assert_array_equal(out["mask"][p, :M], r["mask"], err_msg=f"pair {p}")
        np.testing.assert_array_equal(out["F"][p].view(u), r["F"].view(u), err_msg=f"pair {p}")
        np.testing.assert_array_equal(out["norm"][p].view(u), r["norm"].view(u), err_msg=f"pair {p}")


def _matched(ctx, s, pairs):
    import torch
    pr = _T(np.asarray(pairs, np.int32))
    cnt, mt, _ = ctx.match_batch(_T(s["desc"]), _T(s["n_kp"]), pr, ratio=(4, 5))
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), mt.cpu().numpy()


def test_pilot_settings_agree(ctx):
    """No pilot, one pilot wave per pair, the first block as the pilot: identical outputs on all
    28 pairs, and a sample equals the oracle."""
    s = synth.make_scene(8, 1024, seed=12)
    pairs = synth.unordered_pairs(8)
    cnt, mt = _matched(ctx, s, pairs)
    outs = []
    for v in (0, 64, 256):
        with _pilot(v):
            outs.append(_batch(ctx, s["kps"], pairs, cnt, mt, 1024))
    _same(outs[1], outs[0], cnt)
    _same(outs[2], outs[0], cnt)
    for p in range(0, len(pairs), 5):
        a, b = pairs[p]
        M = cnt[p]
        r = O.ransac_f(s["kps"][a][mt[p, :M, 0]], s["kps"][b][mt[p, :M, 1]], H=1024, seed=42,
                       pa=int(a), pb=int(b))
        _vs_oracle(outs[1], p, r, M)


@pytest.mark.parametrize("n_pairs", [1, 9])
def test_pilot_smallest_grids(ctx, n_pairs):
    """H = 256: the pilot wave is wave 0 of the pair's only block and the second launch has three
    live waves; 1 and 9 pairs leave padding blocks in both launches' grids and a short last XCD."""
    s = synth.make_scene(5, 512, seed=3)
    pairs = synth.unordered_pairs(5)[:n_pairs]
    cnt, mt = _matched(ctx, s, pairs)
    out = _batch(ctx, s["kps"], pairs, cnt, mt, 256)
    for p, (a, b) in enumerate(pairs):
        M = cnt[p]
        r = O.ransac_f(s["kps"][a][mt[p, :M, 0]], s["kps"][b][mt[p, :M, 1]], H=256, seed=42,
                       pa=int(a), pb=int(b))
        _vs_oracle(out, p, r, M)


_pair_cache = {}


def _two_view():
    if not _pair_cache:
        s = synth.make_scene(2, 2048, seed=33)
        q, t, _ = O.match(s["desc"][0], s["desc"][1], 0, 1, (4, 5))
        assert len(q) >= 300
        _pair_cache.update(s=s, q=q, t=t)
    return _pair_cache["s"], _pair_cache["q"], _pair_cache["t"]


@pytest.mark.parametrize("M", [7, 8, 127, 128, 129, 144, 145, 161, 300])
def test_pilot_window_edges_vs_all_counts(ctx, M):
    """Match counts around the preview (for M <= 128 the pilot publishes a preview-only key) and
    the scoring chunks: the batch winner is (max, lowest argmax) over EVERY hypothesis's count,
    the oracle's and the unpruned GPU diagnostic's, and equals O.ransac_f."""
    import torch
    s, q, t = _two_view()
    k_max, H = 2048, 512
    match = np.zeros((1, k_max, 2), np.int32)
    match[0, :M, 0] = q[:M]
    match[0, :M, 1] = t[:M]
    pairs = np.array([[0, 1]], np.int32)
    out = _batch(ctx, s["kps"], pairs, [M], match, H)
    if M < 8:
        assert out["inl_count"][0] == -1 and out["best_h"][0] == -1
        return
    x1, x2 = s["kps"][0][q[:M]], s["kps"][1][t[:M]]
    counts = O.ransac_counts(x1, x2, H=H, seed=42, pa=0, pb=1, thr=1.0)
    gc, _ = ctx.ransac_counts(_T(s["kps"]), _T(pairs), _T(np.array([M], np.int32)), _T(match),
                              n_hyp=H)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(gc.cpu().numpy()[0], counts)
    assert out["inl_count"][0] == counts.max()
    assert out["best_h"][0] == int(np.argmax(counts))     # argmax: the lowest h at the maximum
    _vs_oracle(out, 0, O.ransac_f(x1, x2, H=H, seed=42, pa=0, pb=1), M)


@pytest.mark.parametrize("M,min_ties", [(8, 65), (9, 65), (13, 2)])
def test_pilot_ties_outside_the_pilot(ctx, M, min_ties):
    """Few matches: at M = 8 and 9 more hypotheses tie at the maximum (1024 and 108 of 1024) than
    one pilot wave holds, and the order kernel's atomics decide which of them sit in ranks 0..63;
    at M = 13 the 23 tied all sit in the pilot wave.  The same pair 64 times in one batch: every
    copy returns the oracle's winner, the lowest h among the tied."""
    s, q, t = _two_view()
    k_max, H, P = 2048, 1024, 64
    x1, x2 = s["kps"][0][q[:M]], s["kps"][1][t[:M]]
    counts = O.ransac_counts(x1, x2, H=H, seed=42, pa=0, pb=1, thr=1.0)
    assert (counts == counts.max()).sum() >= min_ties, "the case needs its ties"
    match = np.zeros((P, k_max, 2), np.int32)
    match[:, :M, 0] = q[:M]
    match[:, :M, 1] = t[:M]
    pairs = np.tile(np.array([[0, 1]], np.int32), (P, 1))
    out = _batch(ctx, s["kps"], pairs, [M] * P, match, H)
    r = O.ransac_f(x1, x2, H=H, seed=42, pa=0, pb=1)
    assert r["best_h"] == int(np.argmax(counts))
    for p in range(P):
        _vs_oracle(out, p, r, M)


def test_pilot_counters(ctx):
    """sfm_ransac_stats with the pilot on: every wave is scored by exactly one of the two launches,
    the pilot wave (rank 0..63) of a pair runs to the end (nothing is published before it), no
    wave scores more than M - PV matches, and the executed count keeps its bounds and identity."""
    import torch
    PV, H = 128, 1024
    s = synth.make_scene(7, 2048, seed=5)
    pairs = synth.unordered_pairs(7)
    pr = _T(np.asarray(pairs, np.int32))
    cnt, mt, _ = ctx.match_batch(_T(s["desc"]), _T(s["n_kp"]), pr, ratio=(4, 5))
    cnt[0], cnt[1], cnt[2] = 5, 100, 128          # M < 8, M < PV, M == PV
    with _pilot(None):
        ctx.ransac_stats(enable=True, read=True)      # reset
        try:
            ctx.ransac_batch(_T(s["kps"]), pr, cnt, mt, n_hyp=H, seed=42, thr=1.0)
            stops = ctx.ransac_wave_stops(len(pairs), H).astype(np.int64)
        finally:
            ex, al, npairs = ctx.ransac_stats(enable=False, read=True)
    torch.cuda.synchronize()
    M = cnt.cpu().numpy().astype(np.int64)
    sel = M >= 8
    past = np.maximum(M - PV, 0)
    assert npairs == sel.sum() and al == H * M[sel].sum()
    np.testing.assert_array_equal(stops[sel, 0], past[sel])          # the pilot waves
    assert (stops[sel] <= past[sel, None]).all()
    assert ex == (H * np.minimum(PV, M[sel]) + 64 * stops[sel].sum(1) + M[sel]).sum()
    assert (H * np.minimum(PV, M[sel]) + M[sel]).sum() <= ex <= (H * M[sel] + M[sel]).sum()


def test_pilot_f64_small_pairs(ctx):
    """fp64 mode (the same template) on the small / ragged pairs of
    test_ransac_f64_small_pairs_bit_exact: pilot on and off identical, and equal to the oracle."""
    s = synth.make_scene(4, 700, seed=31)
    pairs = np.array([[0, 1], [1, 2], [2, 3], [0, 3]], np.int32)
    n_keep = [700, 8, 5, 129]
    k_max = 700
    cnt = []
    match = np.zeros((len(pairs), k_max, 2), np.int32)
    for p, (a, b) in enumerate(pairs):
        q, t, _ = O.match(s["desc"][a], s["desc"][b], 0, 1, (4, 5))
        m = min(len(q), n_keep[p])
        match[p, :m] = np.c_[q[:m], t[:m]]
        cnt.append(m)
    kps64 = s["kps"].astype(np.float64)
    outs = []
    for v in (None, 0):
        with _pilot(v):
            outs.append(_batch(ctx, kps64, pairs, cnt, match, 512, seed=7))
    _same(outs[0], outs[1], [m if m >= 8 else 0 for m in cnt])
    for p, (a, b) in enumerate(pairs):
        m = cnt[p]
        x1 = s["kps"][a][match[p, :m, 0]].astype(np.float64)
        x2 = s["kps"][b][match[p, :m, 1]].astype(np.float64)
        o = O.ransac_f(x1, x2, H=512, seed=7, pa=int(a), pb=int(b), f64=True)
        _vs_oracle(outs[0], p, o, m, f64=True)
