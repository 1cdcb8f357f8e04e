// Device helpers shared by the two-view RANSAC kernel families: ransac.hip (fundamental matrix,
// DESIGN.md §4.2) and ransac_h.hip (homography).  Everything here is internal
// to the including translation unit (anonymous namespace / static), so each file compiles its own
// copies with its own flags.
#pragma once

#include <algorithm>
#include <cstdlib>

#include "sfm_internal.h"

namespace {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        // one 32x32->64 product per multiplier (v_mad_u64_u32) instead of mul_hi + mul_lo
        const uint64_t m0 = (uint64_t)0xD2511F53u * c0, m1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(m0 >> 32), lo0 = (uint32_t)m0;
        const uint32_t hi1 = (uint32_t)(m1 >> 32), lo1 = (uint32_t)m1;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Scalar-type helpers: the f32 spec (default) and its fp64 mode (sfm_ransac_f_batch_f64) run the
// same op sequence; these pick the fmaf / fma families (oracle/sfm_oracle_ransac.inc).
__device__ __forceinline__ float fmaT(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double fmaT(double a, double b, double c) { return fma(a, b, c); }
__device__ __forceinline__ float sqrtT(float a) { return sqrtf(a); }
__device__ __forceinline__ double sqrtT(double a) { return sqrt(a); }
__device__ __forceinline__ float fabsT(float a) { return fabsf(a); }
__device__ __forceinline__ double fabsT(double a) { return fabs(a); }
__device__ __forceinline__ float fmaxT(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double fmaxT(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float frexpT(float a, int* e) { return frexpf(a, e); }
__device__ __forceinline__ double frexpT(double a, int* e) { return frexp(a, e); }
__device__ __forceinline__ float ldexpT(float a, int e) { return ldexpf(a, e); }
__device__ __forceinline__ double ldexpT(double a, int e) { return ldexp(a, e); }
template <typename T> struct V4 { T x, y, z, w; };
template <typename T> struct alignas(2 * sizeof(T)) V2 { T x, y; };

// pl[i] through a 32-bit byte offset (the plane block of a pair is < 4 GB): the load takes the
// pair's uniform base in SGPRs and no per-lane 64-bit address arithmetic
template <typename T>
__device__ __forceinline__ T ldT(const T* __restrict__ pl, int i) {
    return *(const T*)((const char*)pl + (uint32_t)i * (uint32_t)sizeof(T));
}

// Null vector z of an 8x9 system by Householder QR of its transpose (oracle_fit_f8's first half):
// Mt[c][k] = entry c of equation k; V[k][r] (r > k) lives in Mt[r][k].  Returns false if a column
// norm vanishes (degenerate sample).  Mt is overwritten.
template <typename T>
__device__ __forceinline__ bool qr_null_8x9(T Mt[9][8], T z[9]) {
    T vkk[8], beta[8];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        T nrm2 = T(0.0);
#pragma unroll
        for (int r = k; r < 9; ++r) nrm2 = fmaT(Mt[r][k], Mt[r][k], nrm2);
        ok = ok && (nrm2 > T(0.0));
        const T nrm = sqrtT(nrm2);
        const T alpha = (Mt[k][k] > T(0.0)) ? -nrm : nrm;
        vkk[k] = Mt[k][k] - alpha;
        T vn2 = fmaT(vkk[k], vkk[k], T(0.0));
#pragma unroll
        for (int r = k + 1; r < 9; ++r) vn2 = fmaT(Mt[r][k], Mt[r][k], vn2);
        ok = ok && (vn2 > T(0.0));
        beta[k] = T(2.0) / vn2;
        Mt[k][k] = alpha;
#pragma unroll
        for (int c = k + 1; c < 8; ++c) {
            T dot = fmaT(vkk[k], Mt[k][c], T(0.0));
#pragma unroll
            for (int r = k + 1; r < 9; ++r) dot = fmaT(Mt[r][k], Mt[r][c], dot);
            const T f = beta[k] * dot;
            Mt[k][c] = fmaT(-f, vkk[k], Mt[k][c]);
#pragma unroll
            for (int r = k + 1; r < 9; ++r) Mt[r][c] = fmaT(-f, Mt[r][k], Mt[r][c]);
        }
    }
    z[0] = z[1] = z[2] = z[3] = z[4] = z[5] = z[6] = z[7] = T(0.0);
    z[8] = T(1.0);
#pragma unroll
    for (int k = 7; k >= 0; --k) {
        T dot = fmaT(vkk[k], z[k], T(0.0));
#pragma unroll
        for (int r = k + 1; r < 9; ++r) dot = fmaT(Mt[r][k], z[r], dot);
        const T f = beta[k] * dot;
        z[k] = fmaT(-f, vkk[k], z[k]);
#pragma unroll
        for (int r = k + 1; r < 9; ++r) z[r] = fmaT(-f, Mt[r][k], z[r]);
    }
    return ok;
}

// per-pair scales of the scoring coordinates (oracle sampson_scales)
template <typename T>
__device__ __forceinline__ void sampson_scales(T s1, T s2, T thr, T& k1, T& k2) {
    const T rt = sqrtT(thr);
    k1 = T(1.0) / (s1 * rt);
    k2 = T(1.0) / (s2 * rt);
}

// fixed-order sum: lane l accumulates m = l, l+64, ... then a halving tree (oracle fixed_sum)
template <typename T>
__device__ __forceinline__ T wave_fixed_sum(T partial) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) partial = partial + __shfl_down(partial, off, 64);
    return __shfl(partial, 0, 64);
}

// plane stride per pair: 8 planes of k_pl floats (k_pl multiple of 16: 64-B aligned planes)
__host__ __device__ __forceinline__ int plane_len(int k_max) { return (k_max + 15) & ~15; }

// One 256-thread block per pair.  The four waves share the dependent gathers (match index ->
// keypoint) and the final scaling; wave 0 alone forms the sums, lane l accumulating m = l, l+64,
// ... in order then the halving tree (the oracle's fixed_sum), so the bits do not depend on the
// block width.  (One wave per pair spent its life on the gather chain: 28 us at cfg3.)
// MIN_M: the model's minimal sample (8 for F, 4 for H); pairs below it get a zero out_norm.
constexpr int PREP_T = 256;
template <typename T, int MIN_M = 8>
__global__ __launch_bounds__(PREP_T) void ransac_prep_kernel(
    const T* __restrict__ kps, int k_max, const int32_t* __restrict__ pairs,
    const int32_t* __restrict__ match_count, const int32_t* __restrict__ matches, T thr,
    T* __restrict__ planes, T* __restrict__ out_norm) {
    __shared__ T par[8];  // mx1, my1, s1, mx2, my2, s2, k1, k2
    const int p = blockIdx.x, tid = threadIdx.x, l = tid & 63;
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    const int M = match_count[p];
    const int32_t* mt = matches + (size_t)p * k_max * 2;
    const int kp = plane_len(k_max);
    T* X1 = planes + (size_t)p * 8 * kp;  // normalised x1 | y1 | x2 | y2
    T* Y1 = X1 + kp;
    T* X2 = Y1 + kp;
    T* Y2 = X2 + kp;
    T* S = Y2 + kp;                        // scaled X1 | Y1 | X2 | Y2
    if (M < MIN_M) {
        if (tid < 6) out_norm[p * 6 + tid] = T(0.0);
        return;
    }
    // gathers: four matches per thread in flight, raw coordinates to the planes
    for (int m0 = tid; m0 < M; m0 += 4 * PREP_T) {
        int2 id[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int m = m0 + PREP_T * t;
            id[t] = m < M ? *(const int2*)(mt + 2 * m) : make_int2(0, 0);
        }
        V2<T> u[4], v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            u[t] = *(const V2<T>*)(kps + ((size_t)a * k_max + id[t].x) * 2);
            v[t] = *(const V2<T>*)(kps + ((size_t)b * k_max + id[t].y) * 2);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int m = m0 + PREP_T * t;
            if (m < M) { X1[m] = u[t].x; Y1[m] = u[t].y; X2[m] = v[t].x; Y2[m] = v[t].y; }
        }
    }
    __syncthreads();  // the raw planes are visible to the block
    if (tid < 64) {
        T sx1 = 0.f, sy1 = 0.f, sx2 = 0.f, sy2 = 0.f;
#pragma unroll 4
        for (int m = l; m < M; m += 64) {
            sx1 = sx1 + X1[m]; sy1 = sy1 + Y1[m]; sx2 = sx2 + X2[m]; sy2 = sy2 + Y2[m];
        }
        const T fM = (T)M;
        const T mx1 = wave_fixed_sum(sx1) / fM, my1 = wave_fixed_sum(sy1) / fM;
        const T mx2 = wave_fixed_sum(sx2) / fM, my2 = wave_fixed_sum(sy2) / fM;
        T sd1 = 0.f, sd2 = 0.f;
#pragma unroll 4
        for (int m = l; m < M; m += 64) {
            const V4<T> w = {X1[m], Y1[m], X2[m], Y2[m]};
            T dx = w.x - mx1, dy = w.y - my1;
            T q = dx * dx;
            q = fmaT(dy, dy, q);
            sd1 = sd1 + sqrtT(q);
            dx = w.z - mx2; dy = w.w - my2;
            q = dx * dx;
            q = fmaT(dy, dy, q);
            sd2 = sd2 + sqrtT(q);
        }
        const T mean1 = wave_fixed_sum(sd1) / fM, mean2 = wave_fixed_sum(sd2) / fM;
        const T s1 = (mean1 > T(0.0)) ? (T(1.41421356237309515) / mean1) : T(1.0);
        const T s2 = (mean2 > T(0.0)) ? (T(1.41421356237309515) / mean2) : T(1.0);
        T k1, k2;
        sampson_scales(s1, s2, thr, k1, k2);
        if (l == 0) {
            par[0] = mx1; par[1] = my1; par[2] = s1; par[3] = mx2; par[4] = my2; par[5] = s2;
            par[6] = k1; par[7] = k2;
            T* o = out_norm + p * 6;
            o[0] = mx1; o[1] = my1; o[2] = s1; o[3] = mx2; o[4] = my2; o[5] = s2;
        }
    }
    __syncthreads();
    const T mx1 = par[0], my1 = par[1], s1 = par[2], mx2 = par[3], my2 = par[4], s2 = par[5];
    const T k1 = par[6], k2 = par[7];
#pragma unroll 4
    for (int m = tid; m < M; m += PREP_T) {
        const T x1 = (X1[m] - mx1) * s1, y1 = (Y1[m] - my1) * s1;
        const T x2 = (X2[m] - mx2) * s2, y2 = (Y2[m] - my2) * s2;
        X1[m] = x1; Y1[m] = y1; X2[m] = x2; Y2[m] = y2;
        S[m] = x1 * k1;
        S[kp + m] = y1 * k1;
        S[2 * kp + m] = x2 * k2;
        S[3 * kp + m] = y2 * k2;
    }
}

typedef const __attribute__((address_space(4))) float* cfloat_p;  // scalar (constant) loads
typedef const __attribute__((address_space(4))) double* cdouble_p;
template <typename T> struct CPtr { typedef cfloat_p type; };
template <> struct CPtr<double> { typedef cdouble_p type; };

typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 sp(float x) { return f2{x, x}; }

// XCD-aware block mapping of the [pair][hypothesis block] grids (fit, score).  Workgroups are
// dispatched round-robin over the 8 XCDs (block b -> XCD b % 8), each XCD with its own 4 MB L2:
// XCD x gets the contiguous pair range [x*Q, (x+1)*Q) and walks it hypothesis-block-major, so a
// pair's scoring planes are read through ONE L2 (with grid (P, H/256) and P = 1 mod 8, as at
// cfg3, every pair's 16 blocks landed on all 8 XCDs) and every pair's first (best-previewed)
// block still runs before any second block.  Returns false for the padding blocks.
__device__ __forceinline__ bool xcd_pair_block(int n_pairs, int n_hb, int gp, int& p, int& hb) {
    const int Q = (n_pairs + 7) >> 3;
    const int x = (int)(blockIdx.x & 7), j = (int)(blockIdx.x >> 3);
    // the XCD's pairs in groups of gp, hb-major inside a group: the best-previewed block of a pair
    // still runs first, and the group's match planes stay in the XCD's L2 while its blocks run
    const int g = j / (gp * n_hb), r = j - g * gp * n_hb;
    const int gsz = min(gp, Q - g * gp);
    hb = r / gsz;
    p = x * Q + g * gp + (r - hb * gsz);
    return p < n_pairs;
}
static inline unsigned xcd_grid(int n_pairs, int n_hb) { return 8u * (unsigned)((n_pairs + 7) >> 3) * (unsigned)n_hb; }

constexpr int CH = 16;         // matches per scalar-load chunk (4 x s_load_dwordx16)
#ifndef RANSAC_PRUNE_EVERY
#define RANSAC_PRUNE_EVERY 32  // K2 at cfg4 vs 32: 16 and 64 +0.8 %, 128 +2.5 % (ransac_prune_every_ab.txt)
#endif
constexpr int PRUNE_EVERY = RANSAC_PRUNE_EVERY;  // matches between bound checks (multiple of CH)
static_assert(PRUNE_EVERY % CH == 0, "prune period");

}  // namespace

// Pairs per XCD group of the ordered schedule (xcd_pair_block).  Measured (profiles/r02/
// ransac_group_ab.txt): groups of 64 -3.9 % K2 at cfg4 (244 pairs per XCD per launch; the group's
// planes stay in L2), +1-2 % at cfg3 (154 per XCD; bounds publish later) -> 64 above 192 pairs
// per XCD, one group below.  SFM_RANSAC_GROUP overrides (A/B only).
static int ransac_group(int n_pairs) {
    const int q = std::max((n_pairs + 7) >> 3, 1);
    const char* e = getenv("SFM_RANSAC_GROUP");
    const int v = e ? atoi(e) : (q > 192 ? 64 : q);
    return (v <= 0 || v > q) ? q : v;
}

#define RANSAC_CHECK_ARGS(NAME)                                                                    \
    SFM_REQUIRE(ctx && prm, NAME ": ctx/prm is NULL");                                             \
    SFM_REQUIRE(n_pairs >= 0 && n_img >= 0 && k_max >= 0, NAME ": negative size");                 \
    if (n_pairs == 0) return SFM_OK;                                                               \
    SFM_REQUIRE(kps && pairs && match_count && matches, NAME ": NULL array");                      \
    SFM_REQUIRE(prm->n_hyp > 0 && prm->n_hyp % 256 == 0,                                           \
                NAME ": n_hyp must be a positive multiple of 256");                                \
    SFM_REQUIRE(prm->thr > 0.0f, NAME ": thr must be > 0");                                        \
    SFM_REQUIRE(k_max <= 8192, NAME ": k_max > 8192 not supported");                               \
    SFM_REQUIRE(prm->n_hyp / 256 <= 65535, NAME ": n_hyp too large")
