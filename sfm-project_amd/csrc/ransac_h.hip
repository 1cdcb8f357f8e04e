// 4-point homography RANSAC: the second model of two-view geometric
// verification (papers/schoenberger2016sfm.pdf §4.1).  A fundamental matrix is not identifiable on
// a planar scene or under pure rotation; comparing the homography's inlier count with F's tells the
// driver which pairs those are (geometric_verification.classify_two_view).
//
// Three kernels per batch of pairs, in the shape of ransac.hip's single-pass schedule:
//   ransac_prep    (ransac_common.h, minimum 4 matches) Hartley normalisation per side over all M
//                  tentative matches; planes x1|y1|x2|y2 normalised and X1|Y1|X2|Y2 scaled by
//                  k = 1/(s*sqrt(thr)).  out_norm is bit-identical to sfm_ransac_f_batch's.
//   ransac_h_hyp   one LANE per hypothesis: Philox stream 2 -> 4 distinct matches (Floyd), null
//                  vector of the 8x9 DLT system (qr_null_8x9, no rank step), validity (QR ok, H
//                  finite, the 4 sample points on one strict side of the line at infinity), then a
//                  sweep over all M matches counting forward-transfer inliers (11 fma/mul + 1
//                  compare per match, division-free).  Match coordinates are wave-uniform: scalar
//                  loads in 16-match chunks.  Exact pruning every PRUNE_EVERY matches against the
//                  pair's published best; one 64-bit atomicMax per wave.  Blocks are mapped with
//                  xcd_pair_block so a pair's planes stay in one XCD's L2.
//   ransac_h_final one block per pair: recomputes the winner, writes the mask, H and count.
// Inlier test with (u, v, w) = H (x1, y1, 1) in normalised coordinates: sign(w) equals the
// sample's and (u - x2 w)^2 + (v - y2 w)^2 - thr s2^2 w^2 < 0.  The scale is folded in as in the F
// path: G = sgn * (rows 0-1 of H times k2 | row 2), X2 = k2 x2, so the test reads
// (u' - X2 w)^2 + (v' - Y2 w)^2 - w^2 < 0 and w > 0, evaluated as q - w|w| < 0 (h_inlier: the same
// bits where w > 0, rejected like `w > 0` rejects elsewhere).  Every float expression is restated
// op for op by tests/h_ref.c (explicit fmaf, -ffp-contract=off), so results are bit-identical to
// the CPU.
#include "ransac_common.h"

namespace {

// Floyd sample of 4 distinct matches; Philox counter (h, 2, a, b): stream 2, disjoint from the F
// sampler's streams 0 and 1
__device__ __forceinline__ void sample4(uint64_t seed, uint32_t pa, uint32_t pb, uint32_t h, int M,
                                        int idx[4]) {
    uint32_t r[4];
    philox4x32_10(h, 2u, pa, pb, (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t jmax = (uint32_t)(M - 4 + k);
        uint32_t t = __umulhi(r[k], jmax + 1u);
        bool dup = false;
#pragma unroll
        for (int q = 0; q < k; ++q) dup = dup || ((uint32_t)idx[q] == t);
        idx[k] = (int)(dup ? jmax : t);
    }
}

// H (row-major, normalised coordinates, as fitted) from 4 correspondences s[k] = (x, y, x', y').
// Returns validity; sgn = the common strict sign of w = h31 x + h32 y + h33 over the sample.
__device__ __forceinline__ bool fit_h4(const V4<float> s[4], float H[9], int& sgn) {
    float Mt[9][8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float x = s[k].x, y = s[k].y, xp = s[k].z, yp = s[k].w;
        const int a = 2 * k, b = 2 * k + 1;
        Mt[0][a] = x;    Mt[1][a] = y;    Mt[2][a] = 1.0f;
        Mt[3][a] = 0.0f; Mt[4][a] = 0.0f; Mt[5][a] = 0.0f;
        Mt[6][a] = -(xp * x); Mt[7][a] = -(xp * y); Mt[8][a] = -xp;
        Mt[0][b] = 0.0f; Mt[1][b] = 0.0f; Mt[2][b] = 0.0f;
        Mt[3][b] = x;    Mt[4][b] = y;    Mt[5][b] = 1.0f;
        Mt[6][b] = -(yp * x); Mt[7][b] = -(yp * y); Mt[8][b] = -yp;
    }
    bool ok = qr_null_8x9(Mt, H);
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && isfinite(H[i]);
    bool pos = true, neg = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float w = fmaf(H[6], s[k].x, fmaf(H[7], s[k].y, H[8]));
        pos = pos && (w > 0.0f);
        neg = neg && (w < 0.0f);
    }
    sgn = neg ? -1 : 1;
    return ok && (pos || neg);
}

// side-2 scale of the scoring coordinates: sampson_scales' k2 (the prep's scaled planes use it)
__device__ __forceinline__ float transfer_scale(float s2, float thr) {
    return 1.0f / (s2 * sqrtf(thr));
}

// scoring copy of H: scale k2 folded into rows 0-1, the whole matrix times the sample's sign (so
// the side test is w > 0); all zero for an invalid hypothesis (w = 0: no match is an inlier)
__device__ __forceinline__ void h_prep(const float H[9], float k2, int sgn, bool valid, float G[9]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const float g = i < 6 ? H[i] * k2 : H[i];
        G[i] = valid ? (sgn < 0 ? -g : g) : 0.0f;
    }
}

__device__ __forceinline__ int h_inlier(const float G[9], float x1, float y1, float X2, float Y2) {
    const float w = fmaf(G[6], x1, fmaf(G[7], y1, G[8]));
    const float u = fmaf(G[0], x1, fmaf(G[1], y1, G[2]));
    const float v = fmaf(G[3], x1, fmaf(G[4], y1, G[5]));
    const float du = fmaf(-X2, w, u);
    const float dv = fmaf(-Y2, w, v);
    const float q = fmaf(dv, dv, du * du);
    // e = q - w|w| carries the side test in its sign: for w > 0 it is the spec's fmaf(-w, w, q) bit
    // for bit, for w <= 0 it is >= 0 (or NaN) and the match is rejected, as `w > 0` rejects it.
    // |w| is a source modifier, so this saves the second compare and the mask AND per match.
    const float e = fmaf(-w, fabsf(w), q);
    return e < 0.0f ? 1 : 0;
}

// two matches per call with v_pk_fma_f32 / v_pk_mul_f32; each half is the scalar op sequence
__device__ __forceinline__ int h_inlier2(const float G[9], f2 x1, f2 y1, f2 X2, f2 Y2) {
    const f2 w = fma2(sp(G[6]), x1, fma2(sp(G[7]), y1, sp(G[8])));
    const f2 u = fma2(sp(G[0]), x1, fma2(sp(G[1]), y1, sp(G[2])));
    const f2 v = fma2(sp(G[3]), x1, fma2(sp(G[4]), y1, sp(G[5])));
    const f2 du = fma2(-X2, w, u);
    const f2 dv = fma2(-Y2, w, v);
    const f2 q = fma2(dv, dv, du * du);
    // the last op per half as a scalar fma with the |w| modifier (h_inlier); v_pk_fma_f32 has none
    // and two v_fma_f32 issue in the time of one v_pk_fma_f32
    const float ex = fmaf(-w.x, fabsf(w.x), q.x), ey = fmaf(-w.y, fabsf(w.y), q.y);
    return (ex < 0.0f ? 1 : 0) + (ey < 0.0f ? 1 : 0);
}

// sample + fit of hypothesis h of the pair whose planes start at pl; G is the scoring copy
__device__ __forceinline__ bool h_hypothesis(const float* __restrict__ pl, int kp, uint64_t seed,
                                             uint32_t pa, uint32_t pb, uint32_t h, int M, float k2,
                                             float H[9], float G[9]) {
    int idx[4];
    sample4(seed, pa, pb, h, M, idx);
    V4<float> smp[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        smp[k] = {ldT(pl, idx[k]), ldT(pl, kp + idx[k]), ldT(pl, 2 * kp + idx[k]),
                  ldT(pl, 3 * kp + idx[k])};
    int sgn;
    const bool valid = fit_h4(smp, H, sgn);
    h_prep(H, k2, sgn, valid, G);
    return valid;
}

// One lane = one hypothesis; see the file comment.  COUNTS (sfm_ransac_h_counts): no pruning, every
// hypothesis's count to out_counts[p][h] and, if asked, its H (zero if invalid) to
// out_hyp_H[p][h][9].
template <bool PRUNE, bool COUNTS>
__global__ __launch_bounds__(256) void ransac_h_hyp_kernel(
    int n_pairs, int k_max, const int32_t* __restrict__ pairs,
    const int32_t* __restrict__ match_count, const float* __restrict__ planes,
    const float* __restrict__ norm, uint64_t seed, float thr, int n_hyp, int gp,
    unsigned long long* __restrict__ best, int32_t* __restrict__ out_counts,
    float* __restrict__ out_hyp_H) {
    static_assert(!(PRUNE && COUNTS), "the diagnostic scores every hypothesis in full");
    int p, hb;
    if (!xcd_pair_block(n_pairs, n_hyp >> 8, gp, p, hb)) return;
    const int M = match_count[p];
    if (M < 4) return;  // block-uniform
    const int kp = plane_len(k_max);
    const float* pl = planes + (size_t)p * 8 * kp;
    const cfloat_p x1p = (cfloat_p)pl, y1p = (cfloat_p)(pl + kp);                // normalised side 1
    const cfloat_p X2p = (cfloat_p)(pl + 6 * kp), Y2p = (cfloat_p)(pl + 7 * kp);  // scaled side 2
    const uint32_t pa = (uint32_t)pairs[2 * p], pb = (uint32_t)pairs[2 * p + 1];
    const float k2 = transfer_scale(norm[p * 6 + 5], thr);
    const uint32_t h = hb * 256 + threadIdx.x;
    float H[9], G[9];
    const bool valid = h_hypothesis(pl, kp, seed, pa, pb, h, M, k2, H, G);
    if (COUNTS && out_hyp_H) {
        float* o = out_hyp_H + ((size_t)p * n_hyp + h) * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) o[k] = valid ? H[k] : 0.0f;  // invalid: zero, as out_H
    }

    int cnt = 0;
    const int Mc = M & ~(CH - 1);
    int m = 0;
    // The published best is read one prune period ahead of its use: a stale value is still a lower
    // bound on the winning count (best[p] only grows), and the load's latency hides behind a
    // period's arithmetic instead of stalling the wave at every check.
    // Only the key's high word (count + 1) is read: it never decreases either, and a one-register
    // destination keeps the load in flight across the period.
    const unsigned* best_hi = (const unsigned*)(best + p) + 1;
    unsigned bhi = 0;
    if (PRUNE) bhi = __hip_atomic_load(best_hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll 1
    for (; m < Mc; m += CH) {
        float x1[CH], y1[CH], X2[CH], Y2[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            x1[j] = x1p[m + j];
            y1[j] = y1p[m + j];
            X2[j] = X2p[m + j];
            Y2[j] = Y2p[m + j];
        }
#pragma unroll
        for (int j = 0; j < CH; j += 2)
            cnt += h_inlier2(G, f2{x1[j], x1[j + 1]}, f2{y1[j], y1[j + 1]}, f2{X2[j], X2[j + 1]},
                             f2{Y2[j], Y2[j + 1]});
        if (PRUNE && ((m + CH) % PRUNE_EVERY) == 0) {
            // Exact pruning: best[p] only grows and every published key is a real hypothesis's
            // (count, id), so (key >> 32) - 1 is a lower bound on the winning count.  A wave
            // whose lanes all satisfy count + remaining < bound holds no possible winner (an
            // invalid lane counts 0 here and -1 in the end, so the test is safe for it too).
            const int bound = (int)bhi - 1;
            if (__all(cnt + (M - m - CH) < bound)) return;  // wave-uniform exit
            bhi = __hip_atomic_load(best_hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
#pragma unroll 1
    for (; m < M; ++m) cnt += h_inlier(G, x1p[m], y1p[m], X2p[m], Y2p[m]);
    if (!valid) cnt = -1;
    if (COUNTS) {
        out_counts[(size_t)p * n_hyp + h] = cnt;
        return;
    }
    unsigned long long key = ((unsigned long long)(unsigned)(cnt + 1) << 32) | (0xFFFFFFFFu - h);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(&best[p], key);  // per wave: later waves prune sooner
}

__global__ __launch_bounds__(256) void ransac_h_final_kernel(
    int k_max, const int32_t* __restrict__ pairs, const int32_t* __restrict__ match_count,
    const float* __restrict__ planes, const float* __restrict__ norm, uint64_t seed, float thr,
    const unsigned long long* __restrict__ best, int32_t* __restrict__ out_inl_count,
    int32_t* __restrict__ out_best_h, uint8_t* __restrict__ out_mask, float* __restrict__ out_H) {
    __shared__ int wsum[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int M = match_count[p];
    uint8_t* mask = out_mask + (size_t)p * k_max;
    // the whole row is written: zero past the pair's matches (and everywhere below 4 matches)
    for (int m = (M < 4 ? 0 : M) + tid; m < k_max; m += 256) mask[m] = 0;
    if (M < 4) {
        if (tid < 9) out_H[p * 9 + tid] = 0.0f;
        if (tid == 0) { out_inl_count[p] = -1; out_best_h[p] = -1; }
        return;
    }
    const uint32_t pa = (uint32_t)pairs[2 * p], pb = (uint32_t)pairs[2 * p + 1];
    const uint32_t h = 0xFFFFFFFFu - (uint32_t)best[p];
    const int kp = plane_len(k_max);
    const float* pl = planes + (size_t)p * 8 * kp;
    const float k2 = transfer_scale(norm[p * 6 + 5], thr);
    float H[9], G[9];
    const bool valid = h_hypothesis(pl, kp, seed, pa, pb, h, M, k2, H, G);
    int cnt = 0;
    for (int m = tid; m < M; m += 256) {
        const int in = h_inlier(G, pl[m], pl[kp + m], pl[6 * kp + m], pl[7 * kp + m]);
        mask[m] = (uint8_t)in;
        cnt += in;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        out_inl_count[p] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        out_best_h[p] = (int)h;
    }
    if (tid < 9) out_H[p * 9 + tid] = valid ? H[tid] : 0.0f;
}

#ifdef RANSAC_H_ABL_NOPRUNE  // ablation build: the batch without pruning (same results; timing only)
constexpr bool H_PRUNE = false;
#else
constexpr bool H_PRUNE = true;
#endif

// workspace of one batch: the 8 planes per pair and the winner keys
int ransac_h_ws(sfm_ctx* ctx, int n_pairs, int kp, float*& planes, unsigned long long*& best) {
    const size_t plb = sfm::align_up((size_t)n_pairs * 8 * kp * sizeof(float), 256);
    const size_t bb = sfm::align_up((size_t)n_pairs * sizeof(unsigned long long), 256);
    char* ws = (char*)sfm::workspace(ctx, plb + bb + 1024);
    if (!ws) return SFM_ERR_NOMEM;
    planes = (float*)ws;
    best = (unsigned long long*)(ws + plb);
    return SFM_OK;
}

}  // namespace

extern "C" int sfm_ransac_h_batch(sfm_ctx* ctx, const float* kps, int32_t n_img, int32_t k_max,
                                  const int32_t* pairs, int32_t n_pairs,
                                  const int32_t* match_count, const int32_t* matches,
                                  const sfm_ransac_params* prm, int32_t* out_inl_count,
                                  int32_t* out_best_h, uint8_t* out_mask, float* out_H,
                                  float* out_norm) {
    RANSAC_CHECK_ARGS("sfm_ransac_h_batch");
    SFM_REQUIRE(out_inl_count && out_best_h && out_mask && out_H && out_norm,
                "sfm_ransac_h_batch: NULL output");
    SFM_REQUIRE(prm->n_hyp <= 65536, "sfm_ransac_h_batch: n_hyp > 65536");
    SFM_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int kp = plane_len(std::max(k_max, 1));
    const int H = prm->n_hyp;
    float* planes;
    unsigned long long* best;
    const int rc = ransac_h_ws(ctx, n_pairs, kp, planes, best);
    if (rc != SFM_OK) return rc;
    SFM_HIP_CHECK(hipMemsetAsync(best, 0, (size_t)n_pairs * sizeof(unsigned long long), st));
    hipLaunchKernelGGL((ransac_prep_kernel<float, 4>), dim3(n_pairs), dim3(PREP_T), 0, st, kps,
                       k_max, pairs, match_count, matches, prm->thr, planes, out_norm);
    SFM_HIP_CHECK(hipGetLastError());
    const dim3 xgrid(xcd_grid(n_pairs, H / 256));
    const int gp = ransac_group(n_pairs);
    hipLaunchKernelGGL((ransac_h_hyp_kernel<H_PRUNE, false>), xgrid, dim3(256), 0, st, n_pairs,
                       k_max, pairs, match_count, planes, out_norm, prm->seed, prm->thr, H, gp,
                       best, (int32_t*)nullptr, (float*)nullptr);
    SFM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ransac_h_final_kernel, dim3(n_pairs), dim3(256), 0, st, k_max, pairs,
                       match_count, planes, out_norm, prm->seed, prm->thr, best, out_inl_count,
                       out_best_h, out_mask, out_H);
    SFM_HIP_CHECK(hipGetLastError());
    return SFM_OK;
}

extern "C" int sfm_ransac_h_counts(sfm_ctx* ctx, const float* kps, int32_t n_img, int32_t k_max,
                                   const int32_t* pairs, int32_t n_pairs,
                                   const int32_t* match_count, const int32_t* matches,
                                   const sfm_ransac_params* prm, int32_t* out_counts,
                                   float* out_norm, float* out_hyp_H) {
    RANSAC_CHECK_ARGS("sfm_ransac_h_counts");
    SFM_REQUIRE(out_counts && out_norm, "sfm_ransac_h_counts: NULL output");
    SFM_REQUIRE(prm->n_hyp <= 65536, "sfm_ransac_h_counts: n_hyp > 65536");
    SFM_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int kp = plane_len(std::max(k_max, 1));
    const int H = prm->n_hyp;
    float* planes;
    unsigned long long* best;
    const int rc = ransac_h_ws(ctx, n_pairs, kp, planes, best);
    if (rc != SFM_OK) return rc;
    // pairs with fewer than 4 matches: every count -1, every H zero
    SFM_HIP_CHECK(hipMemsetAsync(out_counts, 0xFF, (size_t)n_pairs * H * sizeof(int32_t), st));
    if (out_hyp_H)
        SFM_HIP_CHECK(hipMemsetAsync(out_hyp_H, 0, (size_t)n_pairs * H * 9 * sizeof(float), st));
    hipLaunchKernelGGL((ransac_prep_kernel<float, 4>), dim3(n_pairs), dim3(PREP_T), 0, st, kps,
                       k_max, pairs, match_count, matches, prm->thr, planes, out_norm);
    SFM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((ransac_h_hyp_kernel<false, true>), dim3(xcd_grid(n_pairs, H / 256)),
                       dim3(256), 0, st, n_pairs, k_max, pairs, match_count, planes, out_norm,
                       prm->seed, prm->thr, H, ransac_group(n_pairs), best, out_counts, out_hyp_H);
    SFM_HIP_CHECK(hipGetLastError());
    return SFM_OK;
}
