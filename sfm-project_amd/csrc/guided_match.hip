// Guided matching: re-match verified pairs inside the epipolar band of their F.
// L2 / 128-byte descriptors only.  tests/guided_ref.c states the spec; every output equals it
// byte for byte, whatever the batch.
//
// The distances are K1's exact i8 formulation, as sfm_vocab_assign runs it (retrieval.hip): with
// x' = x ^ 0x80, d^2(x, w) = |x'|^2 - vr, vr = 2 x'.w' - |w'|^2, the dot products on
// v_mfma_i32_32x32x32_i8 and the row key 128 vr + (127 - j mod 128), so a max over a 128-row group
// is (largest vr, lowest j) and groups merge in ascending order with a strict compare.
//
// What is new: every accumulator is masked by the Sampson test of K2 before it enters the max.
// cand(i, j) = sampson_inlier(G, X1_i, Y1_i, X2_j, Y2_j) factors into terms of i alone
// (a0, a1, c2), terms of j alone (X2, Y2, bb) and 5 fused multiply-adds per element; the op
// sequence is the oracle's, so the decision is the same bit K2 would take for that match.
//
//   guided_prep_kernel   once per call and image: i8 rows, key constants, |x'|^2; rows from
//                        n_kp[img] up to the 128-padded length are zero with crow = ROW_PAD
//   guided_scan_kernel   one 256-thread workgroup per (pair, 512 queries): the queries are the
//                        MFMA B operand in registers, the other image streams through LDS in
//                        128-row groups together with its key constants and geometric terms.
//                        <false>: queries = image a; masked top-2 (nn, d1, d2) and ncand per i.
//                        <true>:  queries = image b; masked winner rnn per j (mutual rule only).
//                        The Sampson operands keep their FMA positions in both directions.
//   guided_pick_kernel   one workgroup per pair: the rules of oracle_match's non-OpenCV branch and
//                        the compaction to ascending i; writes count and the ncand row.
// A skipped pair leaves the scan kernels block-uniformly before any barrier.  A padded or
// out-of-range row carries NaN terms, so it is never a candidate, and a non-candidate's key is
// INT_MIN, below every real key (|128 vr| < 2^30).
#include <climits>

#include "sfm_internal.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int D = 128;
constexpr int GM_WAVES = 4;
constexpr int GM_QT = 4;                        // query tiles of 32 per wave
constexpr int GM_QB = GM_WAVES * GM_QT * 32;    // 512 queries per workgroup
constexpr int GM_GROUP = 128;                   // streamed rows per LDS stage = one key group
constexpr int GM_NK = D / 32;
constexpr int GM_MAX_KMAX = 8192;
constexpr int ROW_PAD = -(3 << 29);
constexpr int V_NONE = INT_MIN >> 7;            // vr of "no candidate": below every real vr
// one LDS stage: rows | crow | three planes of geometric terms
constexpr int GM_OFF_C = GM_GROUP * D;
constexpr int GM_OFF_T = GM_OFF_C + GM_GROUP * 4;
constexpr int GM_STAGE = GM_OFF_T + 3 * GM_GROUP * 4;

__device__ __forceinline__ int swz(int row) { return (row >> 1) & 7; }

struct GuidedRules {
    int xc, num, den, min_inl;
    long long max_dist;
    float thr;
};

// The pair's geometry: skip rule, image sizes and G (oracle sampson_scales + sampson_prep).
struct PairGeo {
    int a, b, Ka, Kb;
    float cx1, cy1, s1, cx2, cy2, s2, k1, k2, G[9];
    bool skip;
};
__device__ __forceinline__ PairGeo pair_geo(int p, const int32_t* __restrict__ pairs,
                                            const int32_t* __restrict__ n_kp, int k_max,
                                            const int32_t* __restrict__ inl_count,
                                            const float* __restrict__ F,
                                            const float* __restrict__ norm, float thr, int min_inl) {
    PairGeo g;
    g.a = pairs[2 * p];
    g.b = pairs[2 * p + 1];
    g.Ka = min(max(n_kp[g.a], 0), k_max);
    g.Kb = min(max(n_kp[g.b], 0), k_max);
    const float* nr = norm + (size_t)p * 6;
    g.cx1 = nr[0]; g.cy1 = nr[1]; g.s1 = nr[2]; g.cx2 = nr[3]; g.cy2 = nr[4]; g.s2 = nr[5];
    g.skip = inl_count[p] < max(min_inl, 8) || g.Ka == 0 || g.Kb == 0 || g.s1 == 0.0f ||
             g.s2 == 0.0f;
    const float rt = sqrtf(thr);
    g.k1 = 1.0f / (g.s1 * rt);
    g.k2 = 1.0f / (g.s2 * rt);
    const float* f = F + (size_t)p * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) g.G[i] = f[i];
    g.G[2] = f[2] * g.k1;
    g.G[5] = f[5] * g.k1;
    g.G[6] = f[6] * g.k2;
    g.G[7] = f[7] * g.k2;
    g.G[8] = (f[8] * g.k1) * g.k2;
    return g;
}

// terms of a keypoint of image a: (a0, a1, c2)
__device__ __forceinline__ void terms_a(const PairGeo& g, float x, float y, float& t0, float& t1,
                                        float& t2) {
    const float X = ((x - g.cx1) * g.s1) * g.k1, Y = ((y - g.cy1) * g.s1) * g.k1;
    t0 = fmaf(g.G[0], X, fmaf(g.G[1], Y, g.G[2]));
    t1 = fmaf(g.G[3], X, fmaf(g.G[4], Y, g.G[5]));
    t2 = fmaf(g.G[6], X, fmaf(g.G[7], Y, g.G[8]));
}
// terms of a keypoint of image b: (X2, Y2, bb)
__device__ __forceinline__ void terms_b(const PairGeo& g, float x, float y, float& t0, float& t1,
                                        float& t2) {
    const float X = ((x - g.cx2) * g.s2) * g.k2, Y = ((y - g.cy2) * g.s2) * g.k2;
    const float b0 = fmaf(g.G[0], X, fmaf(g.G[3], Y, g.G[6]));
    const float b1 = fmaf(g.G[1], X, fmaf(g.G[4], Y, g.G[7]));
    t0 = X;
    t1 = Y;
    t2 = fmaf(b0, b0, b1 * b1);
}
// the per-element part of sampson_inlier: 5 FMAs and the compare (a NaN gives false)
__device__ __forceinline__ bool cand_elem(float a0, float a1, float c2, float X2, float Y2,
                                          float bb) {
    const float r = fmaf(X2, a0, fmaf(Y2, a1, c2));
    const float den = fmaf(a0, a0, fmaf(a1, a1, bb));
    const float e = fmaf(-r, r, den);
    return e > 0.0f;
}

__global__ __launch_bounds__(256) void guided_prep_kernel(const uint8_t* __restrict__ desc,
                                                          const int32_t* __restrict__ n_kp,
                                                          int k_max, int kpad,
                                                          uint4* __restrict__ desc_i8,
                                                          int32_t* __restrict__ crow,
                                                          int32_t* __restrict__ qn) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, img = blockIdx.y;
    if (j >= kpad) return;
    const size_t o = (size_t)img * kpad + j;
    uint4* o8 = desc_i8 + o * (D / 16);
    if (j >= min(max(n_kp[img], 0), k_max)) {
#pragma unroll
        for (int q = 0; q < D / 16; ++q) o8[q] = make_uint4(0u, 0u, 0u, 0u);
        crow[o] = ROW_PAD;
        qn[o] = 0;
        return;
    }
    const uint4* p = (const uint4*)(desc + ((size_t)img * k_max + j) * D);
    int nv = 0;
#pragma unroll
    for (int q = 0; q < D / 16; ++q) {
        const uint4 v = p[q];
        const uint4 x = make_uint4(v.x ^ 0x80808080u, v.y ^ 0x80808080u, v.z ^ 0x80808080u,
                                   v.w ^ 0x80808080u);
        o8[q] = x;
        nv = __builtin_amdgcn_sdot4((int)x.x, (int)x.x, nv, false);
        nv = __builtin_amdgcn_sdot4((int)x.y, (int)x.y, nv, false);
        nv = __builtin_amdgcn_sdot4((int)x.z, (int)x.z, nv, false);
        nv = __builtin_amdgcn_sdot4((int)x.w, (int)x.w, nv, false);
    }
    crow[o] = -128 * nv + 127 - (j & 127);
    qn[o] = nv;
}

template <bool REV>
__global__ __launch_bounds__(64 * GM_WAVES) void guided_scan_kernel(
    const uint4* __restrict__ desc_i8, const int32_t* __restrict__ crow_tab,
    const int32_t* __restrict__ qn_tab, const int32_t* __restrict__ n_kp,
    const float* __restrict__ kps, int k_max, int kpad, const int32_t* __restrict__ pairs,
    const int32_t* __restrict__ inl_count, const float* __restrict__ F,
    const float* __restrict__ norm, float thr, int min_inl, int n_qb, int32_t* __restrict__ w_nn,
    int32_t* __restrict__ w_d1, int32_t* __restrict__ w_d2, int32_t* __restrict__ w_nc) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][GM_STAGE];
    // block = (pair, 512-query slice), pair-major
    const int p = (int)(blockIdx.x / (unsigned)n_qb), qb = (int)(blockIdx.x % (unsigned)n_qb);
    const PairGeo geo = pair_geo(p, pairs, n_kp, k_max, inl_count, F, norm, thr, min_inl);
    const int qimg = REV ? geo.b : geo.a, timg = REV ? geo.a : geo.b;
    const int Kq = REV ? geo.Kb : geo.Ka, Kt = REV ? geo.Ka : geo.Kb;
    // block-uniform exits, before any barrier
    if (geo.skip || qb * GM_QB >= Kq) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, r32 = lane & 31;
    const int qbase = qb * GM_QB + wave * (GM_QT * 32);
    const int n_group = (Kt + GM_GROUP - 1) / GM_GROUP;

    // the wave's queries: B fragments, geometric terms, running (best vr, its row, second vr,
    // number of candidates)
    v4i bq[GM_QT][GM_NK];
    float q0[GM_QT], q1[GM_QT], q2[GM_QT];
    int B1[GM_QT], J1[GM_QT], B2[GM_QT], NC[GM_QT];
    bool valid[GM_QT];
#pragma unroll
    for (int c = 0; c < GM_QT; ++c) {
        const int q = qbase + c * 32 + r32;
        valid[c] = q < Kq;
        const uint4* src = desc_i8 + ((size_t)qimg * kpad + (valid[c] ? q : 0)) * (D / 16);
#pragma unroll
        for (int s = 0; s < GM_NK; ++s) {
            v4i x = {0, 0, 0, 0};
            if (valid[c]) x = *(const v4i*)(src + 4 * h + s);
            bq[c][s] = x;
        }
        float2 kp = make_float2(0.f, 0.f);
        if (valid[c]) kp = *(const float2*)(kps + ((size_t)qimg * k_max + q) * 2);
        if (REV) terms_b(geo, kp.x, kp.y, q0[c], q1[c], q2[c]);
        else terms_a(geo, kp.x, kp.y, q0[c], q1[c], q2[c]);
        if (!valid[c]) q0[c] = q1[c] = q2[c] = __builtin_nanf("");
        B1[c] = V_NONE; J1[c] = -1; B2[c] = V_NONE; NC[c] = 0;
    }

    // staging: 1024 16-B slots of rows + 32 of constants per group, as sfm_vocab_assign; threads
    // 0..127 also fetch one streamed keypoint each and store its three terms
    uint4 pre0, pre1, pre2, pre3, prec = make_uint4(0u, 0u, 0u, 0u);
    float2 prek = make_float2(0.f, 0.f);
    const bool cthread = tid < GM_GROUP / 4, kthread = tid < GM_GROUP;
    const uint4* tbase = desc_i8 + (size_t)timg * kpad * (D / 16);
    const int32_t* cbase = crow_tab + (size_t)timg * kpad;
    const float* kbase = kps + (size_t)timg * k_max * 2;
#define GM_FETCH(g)                                                                   \
    do {                                                                              \
        const uint4* src_ = tbase + (size_t)(g) * (GM_GROUP * D / 16) + tid;          \
        pre0 = src_[0]; pre1 = src_[256]; pre2 = src_[512]; pre3 = src_[768];         \
        if (cthread) prec = ((const uint4*)(cbase + (size_t)(g) * GM_GROUP))[tid];    \
        if (kthread && (g) * GM_GROUP + tid < Kt)                                     \
            prek = *(const float2*)(kbase + ((size_t)(g) * GM_GROUP + tid) * 2);      \
    } while (0)
    const int st_off = (tid >> 3) * D + (((tid & 7) ^ swz(tid >> 3)) << 4);
#define GM_STORE(dst, g)                                                              \
    do {                                                                              \
        *(uint4*)((dst) + st_off) = pre0;                                             \
        *(uint4*)((dst) + st_off + 32 * D) = pre1;                                    \
        *(uint4*)((dst) + st_off + 64 * D) = pre2;                                    \
        *(uint4*)((dst) + st_off + 96 * D) = pre3;                                    \
        if (cthread) *(uint4*)((dst) + GM_OFF_C + tid * 16) = prec;                   \
        if (kthread) {                                                                \
            float t0_, t1_, t2_;                                                      \
            if (REV) terms_a(geo, prek.x, prek.y, t0_, t1_, t2_);                     \
            else terms_b(geo, prek.x, prek.y, t0_, t1_, t2_);                         \
            if ((g) * GM_GROUP + tid >= Kt) t0_ = t1_ = t2_ = __builtin_nanf("");     \
            float* T_ = (float*)((dst) + GM_OFF_T);                                   \
            T_[tid] = t0_; T_[GM_GROUP + tid] = t1_; T_[2 * GM_GROUP + tid] = t2_;    \
        }                                                                             \
    } while (0)

    GM_FETCH(0);
    GM_STORE(lds[0], 0);
    __syncthreads();
    for (int g = 0; g < n_group; ++g) {
        const unsigned char* A = lds[g & 1];
        const int* Cr = (const int*)(A + GM_OFF_C);
        const float* Tr = (const float*)(A + GM_OFF_T);
        if (g + 1 < n_group) GM_FETCH(g + 1);
        int t1[GM_QT], t2[GM_QT];
#pragma unroll
        for (int c = 0; c < GM_QT; ++c) t1[c] = t2[c] = INT_MIN;
#pragma unroll 1
        for (int tt = 0; tt < GM_GROUP / 32; ++tt) {
            const int row = tt * 32 + r32;
            const int sw = swz(row);
            v4i af[GM_NK];
#pragma unroll
            for (int s = 0; s < GM_NK; ++s)
                af[s] = *(const v4i*)(A + row * D + (((4 * h + s) ^ sw) << 4));
            // accumulator r of lane (., h) is streamed row (r & 3) + 8 (r >> 2) + 4 h of the tile
            int crow[16];
            float s0[16], s1[16], s2[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = tt * 32 + 8 * q + 4 * h;
                const v4i cv = *(const v4i*)(Cr + o);
                const v4f u0 = *(const v4f*)(Tr + o);
                const v4f u1 = *(const v4f*)(Tr + GM_GROUP + o);
                const v4f u2 = *(const v4f*)(Tr + 2 * GM_GROUP + o);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    crow[4 * q + e] = cv[e];
                    s0[4 * q + e] = u0[e]; s1[4 * q + e] = u1[e]; s2[4 * q + e] = u2[e];
                }
            }
#pragma unroll
            for (int c = 0; c < GM_QT; c += 2) {
                v16i acc0 = {0}, acc1 = {0};
#pragma unroll
                for (int s = 0; s < GM_NK; ++s) {
                    acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[s], bq[c][s], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[s], bq[c + 1][s], acc1, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int cc = c + u;
                        const int key = (u ? acc1[r] : acc0[r]) * 256 + crow[r];
                        // image a's terms are (a0, a1, c2), image b's (X2, Y2, bb), whichever
                        // side is the query
                        const bool in = REV ? cand_elem(s0[r], s1[r], s2[r], q0[cc], q1[cc], q2[cc])
                                            : cand_elem(q0[cc], q1[cc], q2[cc], s0[r], s1[r], s2[r]);
                        const int k = in ? key : INT_MIN;
                        if (!REV) {
                            t2[cc] = max(t2[cc], min(t1[cc], k));
                            NC[cc] += in ? 1 : 0;
                        }
                        t1[cc] = max(t1[cc], k);
                    }
                }
            }
        }
        // merge the group: strict compare in ascending group order keeps the lowest index; the
        // second value is the multiset's (an equal best of a later group becomes the second)
#pragma unroll
        for (int c = 0; c < GM_QT; ++c) {
            const int v1 = t1[c] >> 7, v2 = t2[c] >> 7;
            const int j1 = g * GM_GROUP + 127 - (t1[c] & 127);
            if (v1 > B1[c]) { B2[c] = max(B1[c], v2); B1[c] = v1; J1[c] = j1; }
            else B2[c] = max(B2[c], v1);
        }
        if (g + 1 < n_group) GM_STORE(lds[(g + 1) & 1], g + 1);
        __syncthreads();
    }

#pragma unroll
    for (int c = 0; c < GM_QT; ++c) {
        // the other half of the streamed rows lives in lane ^ 32
        const int P1 = __shfl_xor(B1[c], 32), PJ = __shfl_xor(J1[c], 32);
        const int P2 = __shfl_xor(B2[c], 32), PN = __shfl_xor(NC[c], 32);
        if (P1 > B1[c] || (P1 == B1[c] && PJ < J1[c])) {
            B2[c] = max(B1[c], P2); B1[c] = P1; J1[c] = PJ;
        } else {
            B2[c] = max(B2[c], P1);
        }
        const int q = qbase + c * 32 + r32;
        if (h == 0 && valid[c]) {
            const size_t o = (size_t)p * kpad + q;
            const bool any = B1[c] != V_NONE;
            w_nn[o] = any ? J1[c] : -1;
            if (!REV) {
                const int nq = qn_tab[(size_t)qimg * kpad + q];
                w_d1[o] = any ? nq - B1[c] : INT_MAX;          // d^2 = |x'|^2 - vr
                w_d2[o] = B2[c] != V_NONE ? nq - B2[c] : INT_MAX;
                w_nc[o] = NC[c] + PN;
            }
        }
    }
}
#undef GM_FETCH
#undef GM_STORE

// The rules and the compaction, one workgroup per pair; queries in ascending chunks of 256, the
// kept ones placed by a ballot scan, so the output order is ascending i whatever the schedule.
__global__ __launch_bounds__(256) void guided_pick_kernel(
    const int32_t* __restrict__ n_kp, int k_max, int kpad, const int32_t* __restrict__ pairs,
    const int32_t* __restrict__ inl_count, const float* __restrict__ norm, GuidedRules R,
    const int32_t* __restrict__ w_nn, const int32_t* __restrict__ w_d1,
    const int32_t* __restrict__ w_d2, const int32_t* __restrict__ w_nc,
    const int32_t* __restrict__ w_rnn, int32_t* __restrict__ out_count,
    int32_t* __restrict__ out_match, int32_t* __restrict__ out_dist,
    int32_t* __restrict__ out_ncand) {
    __shared__ int wcnt[4];
    const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    const int Ka = min(max(n_kp[a], 0), k_max), Kb = min(max(n_kp[b], 0), k_max);
    const float s1 = norm[(size_t)p * 6 + 2], s2 = norm[(size_t)p * 6 + 5];
    const bool skip = inl_count[p] < max(R.min_inl, 8) || Ka == 0 || Kb == 0 || s1 == 0.0f ||
                      s2 == 0.0f;
    if (out_ncand) {
        int32_t* nc = out_ncand + (size_t)p * k_max;
        for (int i = tid; i < k_max; i += 256)
            nc[i] = (!skip && i < Ka) ? w_nc[(size_t)p * kpad + i] : 0;
    }
    if (skip) {
        if (tid == 0) out_count[p] = 0;
        return;
    }
    const size_t wo = (size_t)p * kpad;
    int32_t* om = out_match + (size_t)p * k_max * 2;
    int32_t* od = out_dist + (size_t)p * k_max;
    int n = 0;
    for (int base = 0; base < Ka; base += 256) {
        const int i = base + tid;
        bool keep = false;
        int j = -1, d1 = 0;
        if (i < Ka) {
            j = w_nn[wo + i];
            if (j >= 0) {
                d1 = w_d1[wo + i];
                const int d2 = w_d2[wo + i];
                keep = R.xc != SFM_XC_MUTUAL || w_rnn[wo + j] == i;
                if (R.den > 0 && d2 != INT_MAX)
                    keep = keep && (long long)R.den * R.den * d1 < (long long)R.num * R.num * d2;
                if (R.max_dist >= 0) keep = keep && (long long)d1 < R.max_dist;
            }
        }
        const unsigned long long bal = __ballot(keep);
        __syncthreads();   // the previous chunk's wcnt has been read
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int off = n, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) off += wcnt[w];
            tot += wcnt[w];
        }
        if (keep) {
            const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
            om[2 * pos] = i;
            om[2 * pos + 1] = j;
            od[pos] = d1;
        }
        n += tot;
    }
    if (tid == 0) out_count[p] = n;
}

}  // namespace

extern "C" int sfm_guided_match_batch(sfm_ctx* ctx, const uint8_t* desc, const int32_t* n_kp,
                                      const float* kps, int32_t n_img, int32_t k_max, int32_t dim,
                                      const int32_t* pairs, int32_t n_pairs,
                                      const int32_t* inl_count, const float* F, const float* norm,
                                      const sfm_guided_params* prm, int32_t* out_count,
                                      int32_t* out_match, int32_t* out_dist, int32_t* out_ncand) {
    SFM_REQUIRE(prm != nullptr, "sfm_guided_match_batch: prm is NULL");
    SFM_REQUIRE(prm->struct_size >= (int32_t)sizeof(sfm_guided_params),
                "sfm_guided_match_batch: prm->struct_size is smaller than the struct");
    SFM_REQUIRE(dim == 128, "sfm_guided_match_batch: L2 descriptors with dim == 128 only "
                            "(Hamming / ORB descriptors are out of scope)");
    SFM_REQUIRE(prm->cross_check != SFM_XC_OPENCV,
                "sfm_guided_match_batch: the OpenCV cross-check rule is not supported "
                "(SFM_XC_NONE or SFM_XC_MUTUAL)");
    SFM_REQUIRE(prm->cross_check == SFM_XC_NONE || prm->cross_check == SFM_XC_MUTUAL,
                "sfm_guided_match_batch: bad cross_check");
    SFM_REQUIRE(prm->ratio_den >= 0 && prm->ratio_num >= 0 && prm->ratio_num <= 65535 &&
                    prm->ratio_den <= 65535,
                "sfm_guided_match_batch: ratio must be num/den with 0 <= num, den <= 65535");
    SFM_REQUIRE(prm->thr > 0.0f && prm->thr < 3.0e38f, "sfm_guided_match_batch: thr must be > 0");
    SFM_REQUIRE(n_pairs >= 0 && n_img >= 0 && k_max >= 0, "sfm_guided_match_batch: negative size");
    SFM_REQUIRE(k_max <= GM_MAX_KMAX, "sfm_guided_match_batch: k_max > 8192 not supported");
    SFM_REQUIRE(ctx != nullptr, "sfm_guided_match_batch: ctx is NULL");
    if (n_pairs == 0) return SFM_OK;
    SFM_REQUIRE(desc && n_kp && kps && pairs && inl_count && F && norm && out_count && out_match &&
                    out_dist,
                "sfm_guided_match_batch: NULL array");
    SFM_REQUIRE(n_img <= 65535, "sfm_guided_match_batch: more than 65535 images");
    SFM_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool mutual = prm->cross_check == SFM_XC_MUTUAL;
    if (k_max == 0 || n_img == 0) {
        SFM_HIP_CHECK(hipMemsetAsync(out_count, 0, (size_t)n_pairs * sizeof(int32_t), st));
        return SFM_OK;
    }
    const int kpad = (int)sfm::align_up((size_t)k_max, GM_GROUP);
    const size_t rows = (size_t)n_img * kpad, prow = (size_t)n_pairs * kpad;
    const size_t b8 = rows * D, bt = rows * sizeof(int32_t), bp = prow * sizeof(int32_t);
    char* ws = (char*)sfm::workspace(ctx, b8 + 2 * bt + 5 * bp);
    if (!ws) return SFM_ERR_NOMEM;
    uint4* desc_i8 = (uint4*)ws;
    int32_t* crow = (int32_t*)(ws + b8);
    int32_t* qn = (int32_t*)(ws + b8 + bt);
    int32_t* w_nn = (int32_t*)(ws + b8 + 2 * bt);
    int32_t *w_d1 = w_nn + prow, *w_d2 = w_d1 + prow, *w_nc = w_d2 + prow, *w_rnn = w_nc + prow;
    hipLaunchKernelGGL(guided_prep_kernel, dim3((kpad + 255) / 256, n_img), dim3(256), 0, st, desc,
                       n_kp, k_max, kpad, desc_i8, crow, qn);
    SFM_HIP_CHECK(hipGetLastError());
    const int n_qb = (k_max + GM_QB - 1) / GM_QB;   // <= 16, so the grid fits 2^31 blocks
    SFM_REQUIRE((long long)n_pairs * n_qb <= INT_MAX, "sfm_guided_match_batch: too many pairs");
    const dim3 grid((unsigned)n_pairs * (unsigned)n_qb);
    hipLaunchKernelGGL(guided_scan_kernel<false>, grid, dim3(64 * GM_WAVES), 0, st, desc_i8, crow,
                       qn, n_kp, kps, k_max, kpad, pairs, inl_count, F, norm, prm->thr,
                       prm->min_inliers, n_qb, w_nn, w_d1, w_d2, w_nc);
    SFM_HIP_CHECK(hipGetLastError());
    if (mutual) {
        hipLaunchKernelGGL(guided_scan_kernel<true>, grid, dim3(64 * GM_WAVES), 0, st, desc_i8,
                           crow, qn, n_kp, kps, k_max, kpad, pairs, inl_count, F, norm, prm->thr,
                           prm->min_inliers, n_qb, w_rnn, (int32_t*)nullptr, (int32_t*)nullptr,
                           (int32_t*)nullptr);
        SFM_HIP_CHECK(hipGetLastError());
    }
    GuidedRules R;
    R.xc = prm->cross_check; R.num = prm->ratio_num; R.den = prm->ratio_den;
    R.min_inl = prm->min_inliers; R.max_dist = prm->max_dist; R.thr = prm->thr;
    hipLaunchKernelGGL(guided_pick_kernel, dim3(n_pairs), dim3(256), 0, st, n_kp, k_max, kpad,
                       pairs, inl_count, norm, R, w_nn, w_d1, w_d2, w_nc, w_rnn, out_count,
                       out_match, out_dist, out_ncand);
    SFM_HIP_CHECK(hipGetLastError());
    return SFM_OK;
}
