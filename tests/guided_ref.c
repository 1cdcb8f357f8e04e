/*
 * guided_ref.c — CPU statement of the guided-matching spec.
 *
 * TEST INFRASTRUCTURE ONLY: tests/guided_ref.py builds and loads it; the product package never
 * does.  sfm_guided_match_batch equals guidedref_batch byte for byte.
 *
 * sampson_scales / sampson_prep / sampson_inlier are copied from oracle/sfm_oracle_ransac.inc
 * (R = float): their op sequence is the spec, and tests/test_guided_ref_cpu.py pins this copy to
 * oracle.ransac_f's inlier mask.  Compiled with -ffp-contract=off: only the explicit fmaf fuse.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define SFM_XC_MUTUAL 1
#define NONE INT64_MAX

static inline void sampson_scales(float s1, float s2, float thr, float* k1, float* k2) {
    const float rt = sqrtf(thr);
    *k1 = 1.0f / (s1 * rt);
    *k2 = 1.0f / (s2 * rt);
}

static inline void sampson_prep(const float F[9], float k1, float k2, float G[9]) {
    for (int i = 0; i < 9; ++i) G[i] = F[i];
    G[2] = F[2] * k1;
    G[5] = F[5] * k1;
    G[6] = F[6] * k2;
    G[7] = F[7] * k2;
    G[8] = (F[8] * k1) * k2;
}

static inline int sampson_inlier(const float G[9], float x1, float y1, float x2, float y2) {
    float a0 = fmaf(G[0], x1, fmaf(G[1], y1, G[2]));
    float a1 = fmaf(G[3], x1, fmaf(G[4], y1, G[5]));
    float c2 = fmaf(G[6], x1, fmaf(G[7], y1, G[8]));
    float b0 = fmaf(G[0], x2, fmaf(G[3], y2, G[6]));
    float b1 = fmaf(G[1], x2, fmaf(G[4], y2, G[7]));
    float r = fmaf(x2, a0, fmaf(y2, a1, c2));
    float den = fmaf(a0, a0, fmaf(a1, a1, fmaf(b0, b0, b1 * b1)));
    float e = fmaf(-r, r, den);
    return e > 0.0f;
}

/* scoring coordinate of one pixel coordinate: ((x - c) * s) * k, each operation rounded */
static inline float coord(float x, float c, float s, float k) {
    float n = (x - c) * s;
    return n * k;
}

static inline int64_t l2sq_u8(const uint8_t* a, const uint8_t* b) {
    int64_t s = 0;
    for (int k = 0; k < 128; ++k) { int d = (int)a[k] - (int)b[k]; s += d * d; }
    return s;
}

/* cand of n point pairs (xy1[m], xy2[m]) in pixels under (F, norm, thr): out[m] = 0 / 1 */
void guidedref_cand(const float* F, const float* norm, float thr, const float* xy1,
                    const float* xy2, int n, uint8_t* out) {
    float k1, k2, G[9];
    sampson_scales(norm[2], norm[5], thr, &k1, &k2);
    sampson_prep(F, k1, k2, G);
    for (int m = 0; m < n; ++m)
        out[m] = (uint8_t)sampson_inlier(G, coord(xy1[2 * m], norm[0], norm[2], k1),
                                         coord(xy1[2 * m + 1], norm[1], norm[2], k1),
                                         coord(xy2[2 * m], norm[3], norm[5], k2),
                                         coord(xy2[2 * m + 1], norm[4], norm[5], k2));
}

/* The batch.  desc [n_img][k_max][128] u8, kps [n_img][k_max][2] f32; outputs as
 * sfm_guided_match_batch (rows zero from count on; out_ncand may be NULL). */
void guidedref_batch(const uint8_t* desc, const int32_t* n_kp, const float* kps, int n_img,
                     int k_max, const int32_t* pairs, int n_pairs, const int32_t* inl_count,
                     const float* F, const float* norm, int cross_check, int ratio_num,
                     int ratio_den, int min_inliers, float thr, int64_t max_dist,
                     int32_t* out_count, int32_t* out_match, int32_t* out_dist,
                     int32_t* out_ncand) {
    (void)n_img;
    const int K = k_max > 0 ? k_max : 1;
    float* X1 = (float*)malloc(sizeof(float) * 2 * K);
    float* X2 = (float*)malloc(sizeof(float) * 2 * K);
    int32_t* nn = (int32_t*)malloc(sizeof(int32_t) * K);
    int32_t* rnn = (int32_t*)malloc(sizeof(int32_t) * K);
    int64_t* d1 = (int64_t*)malloc(sizeof(int64_t) * K);
    int64_t* d2 = (int64_t*)malloc(sizeof(int64_t) * K);
    int64_t* rd = (int64_t*)malloc(sizeof(int64_t) * K);
    for (int p = 0; p < n_pairs; ++p) {
        int32_t* om = out_match + (size_t)p * k_max * 2;
        int32_t* od = out_dist + (size_t)p * k_max;
        int32_t* nc = out_ncand ? out_ncand + (size_t)p * k_max : NULL;
        memset(om, 0, sizeof(int32_t) * 2 * (size_t)k_max);
        memset(od, 0, sizeof(int32_t) * (size_t)k_max);
        if (nc) memset(nc, 0, sizeof(int32_t) * (size_t)k_max);
        out_count[p] = 0;
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        int Ka = n_kp[a], Kb = n_kp[b];
        Ka = Ka < 0 ? 0 : (Ka > k_max ? k_max : Ka);
        Kb = Kb < 0 ? 0 : (Kb > k_max ? k_max : Kb);
        const float* nr = norm + (size_t)p * 6;
        const float cx1 = nr[0], cy1 = nr[1], s1 = nr[2], cx2 = nr[3], cy2 = nr[4], s2 = nr[5];
        const int bar = min_inliers > 8 ? min_inliers : 8;
        if (inl_count[p] < bar || Ka == 0 || Kb == 0 || s1 == 0.0f || s2 == 0.0f) continue;
        float k1, k2, G[9];
        sampson_scales(s1, s2, thr, &k1, &k2);
        sampson_prep(F + (size_t)p * 9, k1, k2, G);
        const float* ka = kps + (size_t)a * k_max * 2;
        const float* kb = kps + (size_t)b * k_max * 2;
        for (int i = 0; i < Ka; ++i) {
            X1[2 * i] = coord(ka[2 * i], cx1, s1, k1);
            X1[2 * i + 1] = coord(ka[2 * i + 1], cy1, s1, k1);
        }
        for (int j = 0; j < Kb; ++j) {
            X2[2 * j] = coord(kb[2 * j], cx2, s2, k2);
            X2[2 * j + 1] = coord(kb[2 * j + 1], cy2, s2, k2);
            rnn[j] = -1;
            rd[j] = NONE;
        }
        const uint8_t* A = desc + (size_t)a * k_max * 128;
        const uint8_t* B = desc + (size_t)b * k_max * 128;
        /* nn_tables of oracle/sfm_oracle.c over the candidates only */
        for (int i = 0; i < Ka; ++i) {
            int64_t b1 = NONE, b2 = NONE;
            int32_t j1 = -1, n = 0;
            for (int j = 0; j < Kb; ++j) {
                if (!sampson_inlier(G, X1[2 * i], X1[2 * i + 1], X2[2 * j], X2[2 * j + 1])) continue;
                ++n;
                const int64_t d = l2sq_u8(A + (size_t)i * 128, B + (size_t)j * 128);
                if (d < b1) { b2 = b1; b1 = d; j1 = j; }
                else if (d < b2) { b2 = d; }
                if (d < rd[j]) { rd[j] = d; rnn[j] = i; }
            }
            nn[i] = j1; d1[i] = b1; d2[i] = b2;
            if (nc) nc[i] = n;
        }
        int n = 0;
        for (int i = 0; i < Ka; ++i) {
            const int j = nn[i];
            if (j < 0) continue;
            if (cross_check == SFM_XC_MUTUAL && rnn[j] != i) continue;
            if (ratio_den > 0 && d2[i] != NONE) {
                __int128 lhs = (__int128)ratio_den * ratio_den * d1[i];
                __int128 rhs = (__int128)ratio_num * ratio_num * d2[i];
                if (!(lhs < rhs)) continue;
            }
            if (max_dist >= 0 && !(d1[i] < max_dist)) continue;
            om[2 * n] = i; om[2 * n + 1] = j; od[n] = (int32_t)d1[i];
            ++n;
        }
        out_count[p] = n;
    }
    free(X1); free(X2); free(nn); free(rnn); free(d1); free(d2); free(rd);
}
