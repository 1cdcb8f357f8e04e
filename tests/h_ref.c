/*
 * CPU restatement of the homography RANSAC spec (TEST INFRASTRUCTURE ONLY; DESIGN.md §4.2a,
 * include/sfmcore.h sfm_ransac_h_batch).  Written from the spec, op for op in f32 with explicit
 * fmaf: its own Philox and sample4, Hartley normalisation with the fixed-order sum, the 8x9 DLT
 * null vector by Householder QR, validity, the division-free forward-transfer test, the winner,
 * and every hypothesis's count and H.  tests/h_ref.py is the ctypes front-end.
 * Build: gcc -O3 -march=x86-64-v3 -ffp-contract=off -fno-fast-math -fPIC -shared.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

void href_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t m0 = (uint64_t)0xD2511F53u * c0, m1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(m1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)m1;
        const uint32_t n2 = (uint32_t)(m0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)m0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

/* Floyd: 4 distinct indices in [0, M), M >= 4; Philox counter (h, 2, pa, pb), key = seed */
void href_sample4(uint64_t seed, uint32_t pa, uint32_t pb, uint32_t h, int32_t M, int32_t idx[4]) {
    const uint32_t ctr[4] = {h, 2u, pa, pb}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t r[4];
    href_philox4x32_10(ctr, key, r);
    for (int k = 0; k < 4; ++k) {
        const uint32_t jmax = (uint32_t)(M - 4 + k);
        const uint32_t t = (uint32_t)(((uint64_t)r[k] * (uint64_t)(jmax + 1u)) >> 32);
        int dup = 0;
        for (int q = 0; q < k; ++q) dup = dup || ((uint32_t)idx[q] == t);
        idx[k] = (int32_t)(dup ? jmax : t);
    }
}

/* 64 lane partials (lane l sums m = l, l+64, ... in order), then a halving tree */
static float fixed_sum(const float* v, int M) {
    float p[64];
    for (int l = 0; l < 64; ++l) {
        float s = 0.0f;
        for (int m = l; m < M; m += 64) s = s + v[m];
        p[l] = s;
    }
    for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l) p[l] = p[l] + p[l + off];
    return p[0];
}

/* Hartley normalisation of one side: xy [M][2] -> nxy [M][2], (cx, cy, s) */
void href_normalize(const float* xy, int32_t M, float* nxy, float* cx, float* cy, float* s) {
    float* tmp = (float*)calloc((size_t)(M > 0 ? M : 1), sizeof(float));
    for (int m = 0; m < M; ++m) tmp[m] = xy[2 * m];
    const float mx = fixed_sum(tmp, M) / (float)M;
    for (int m = 0; m < M; ++m) tmp[m] = xy[2 * m + 1];
    const float my = fixed_sum(tmp, M) / (float)M;
    for (int m = 0; m < M; ++m) {
        const float dx = xy[2 * m] - mx, dy = xy[2 * m + 1] - my;
        float q = dx * dx;
        q = fmaf(dy, dy, q);
        tmp[m] = sqrtf(q);
    }
    const float mean = fixed_sum(tmp, M) / (float)M;
    const float sc = (mean > 0.0f) ? (1.41421356237309515f / mean) : 1.0f;
    for (int m = 0; m < M; ++m) {
        nxy[2 * m] = (xy[2 * m] - mx) * sc;
        nxy[2 * m + 1] = (xy[2 * m + 1] - my) * sc;
    }
    *cx = mx; *cy = my; *s = sc;
    free(tmp);
}

/* null vector of the 8 equations A[k][0..8] by Householder QR of A^T; returns 0 if a column norm
 * vanishes.  Column k of Q's factor lives in a[k..8][k]. */
static int qr_null(float a[9][8], float z[9]) {
    float vkk[8], beta[8];
    int ok = 1;
    for (int k = 0; k < 8; ++k) {
        float nrm2 = 0.0f;
        for (int r = k; r < 9; ++r) nrm2 = fmaf(a[r][k], a[r][k], nrm2);
        ok = ok && (nrm2 > 0.0f);
        const float nrm = sqrtf(nrm2);
        const float alpha = (a[k][k] > 0.0f) ? -nrm : nrm;
        vkk[k] = a[k][k] - alpha;
        float vn2 = fmaf(vkk[k], vkk[k], 0.0f);
        for (int r = k + 1; r < 9; ++r) vn2 = fmaf(a[r][k], a[r][k], vn2);
        ok = ok && (vn2 > 0.0f);
        beta[k] = 2.0f / vn2;
        a[k][k] = alpha;
        for (int c = k + 1; c < 8; ++c) {
            float dot = fmaf(vkk[k], a[k][c], 0.0f);
            for (int r = k + 1; r < 9; ++r) dot = fmaf(a[r][k], a[r][c], dot);
            const float f = beta[k] * dot;
            a[k][c] = fmaf(-f, vkk[k], a[k][c]);
            for (int r = k + 1; r < 9; ++r) a[r][c] = fmaf(-f, a[r][k], a[r][c]);
        }
    }
    for (int i = 0; i < 8; ++i) z[i] = 0.0f;
    z[8] = 1.0f;
    for (int k = 7; k >= 0; --k) {
        float dot = fmaf(vkk[k], z[k], 0.0f);
        for (int r = k + 1; r < 9; ++r) dot = fmaf(a[r][k], z[r], dot);
        const float f = beta[k] * dot;
        z[k] = fmaf(-f, vkk[k], z[k]);
        for (int r = k + 1; r < 9; ++r) z[r] = fmaf(-f, a[r][k], z[r]);
    }
    return ok;
}

/* H from 4 normalised correspondences p1/p2 [4][2]; returns validity (1/0) and the sample's sign */
int32_t href_fit_h4(const float* p1, const float* p2, float H[9], int32_t* sgn) {
    float a[9][8];
    for (int k = 0; k < 4; ++k) {
        const float x = p1[2 * k], y = p1[2 * k + 1], xp = p2[2 * k], yp = p2[2 * k + 1];
        const int e = 2 * k, o = 2 * k + 1;
        a[0][e] = x;    a[1][e] = y;    a[2][e] = 1.0f;
        a[3][e] = 0.0f; a[4][e] = 0.0f; a[5][e] = 0.0f;
        a[6][e] = -(xp * x); a[7][e] = -(xp * y); a[8][e] = -xp;
        a[0][o] = 0.0f; a[1][o] = 0.0f; a[2][o] = 0.0f;
        a[3][o] = x;    a[4][o] = y;    a[5][o] = 1.0f;
        a[6][o] = -(yp * x); a[7][o] = -(yp * y); a[8][o] = -yp;
    }
    int ok = qr_null(a, H);
    for (int i = 0; i < 9; ++i) ok = ok && isfinite(H[i]);
    int pos = 1, neg = 1;
    for (int k = 0; k < 4; ++k) {
        const float w = fmaf(H[6], p1[2 * k], fmaf(H[7], p1[2 * k + 1], H[8]));
        pos = pos && (w > 0.0f);
        neg = neg && (w < 0.0f);
    }
    *sgn = neg ? -1 : 1;
    return ok && (pos || neg);
}

static void h_prep(const float H[9], float k2, int sgn, int valid, float G[9]) {
    for (int i = 0; i < 9; ++i) {
        const float g = i < 6 ? H[i] * k2 : H[i];
        G[i] = valid ? (sgn < 0 ? -g : g) : 0.0f;
    }
}

static int h_inlier(const float G[9], float x1, float y1, float X2, float Y2) {
    const float w = fmaf(G[6], x1, fmaf(G[7], y1, G[8]));
    const float u = fmaf(G[0], x1, fmaf(G[1], y1, G[2]));
    const float v = fmaf(G[3], x1, fmaf(G[4], y1, G[5]));
    const float du = fmaf(-X2, w, u);
    const float dv = fmaf(-Y2, w, v);
    const float q = fmaf(dv, dv, du * du);
    const float e = fmaf(-w, w, q);
    return (e < 0.0f && w > 0.0f) ? 1 : 0;
}

/*
 * RANSAC over one pair.  xy1/xy2 [M][2] pixel coordinates in match order.  Writes every
 * hypothesis's count (-1 invalid) and H (zero if invalid) when the pointers are given, the
 * winner (max count, lowest h), its mask, H (normalised, zero if invalid) and the normalisation.
 * Returns the winner's count, -1 if M < 4 (then best_h -1, zero H / norm / mask, counts -1).
 */
int32_t href_ransac_h(const float* xy1, const float* xy2, int32_t M, int32_t nh, uint64_t seed,
                      uint32_t pa, uint32_t pb, float thr, int32_t* best_h, float Hout[9],
                      float norm[6], uint8_t* mask, int32_t* counts, float* hyp_H) {
    if (M < 4) {
        *best_h = -1;
        memset(Hout, 0, 9 * sizeof(float));
        memset(norm, 0, 6 * sizeof(float));
        for (int m = 0; m < M; ++m) mask[m] = 0;
        if (counts) for (int h = 0; h < nh; ++h) counts[h] = -1;
        if (hyp_H) memset(hyp_H, 0, (size_t)nh * 9 * sizeof(float));
        return -1;
    }
    float* n1 = (float*)malloc(sizeof(float) * 2 * M);
    float* n2 = (float*)malloc(sizeof(float) * 2 * M);
    float* S2 = (float*)malloc(sizeof(float) * 2 * M);
    float cx1, cy1, s1, cx2, cy2, s2;
    href_normalize(xy1, M, n1, &cx1, &cy1, &s1);
    href_normalize(xy2, M, n2, &cx2, &cy2, &s2);
    const float rt = sqrtf(thr);
    const float k2 = 1.0f / (s2 * rt);
    for (int i = 0; i < 2 * M; ++i) S2[i] = n2[i] * k2;
    int bestc = -2, besth = -1;
    float Hb[9];
    int validb = 0, sgnb = 1;
    for (int h = 0; h < nh; ++h) {
        int32_t idx[4], sgn;
        href_sample4(seed, pa, pb, (uint32_t)h, M, idx);
        float p1[8], p2[8], H[9], G[9];
        for (int k = 0; k < 4; ++k) {
            p1[2 * k] = n1[2 * idx[k]]; p1[2 * k + 1] = n1[2 * idx[k] + 1];
            p2[2 * k] = n2[2 * idx[k]]; p2[2 * k + 1] = n2[2 * idx[k] + 1];
        }
        const int valid = href_fit_h4(p1, p2, H, &sgn);
        int cnt = -1;
        if (valid) {
            h_prep(H, k2, sgn, 1, G);
            cnt = 0;
            for (int m = 0; m < M; ++m)
                cnt += h_inlier(G, n1[2 * m], n1[2 * m + 1], S2[2 * m], S2[2 * m + 1]);
        }
        if (counts) counts[h] = cnt;
        if (hyp_H) for (int i = 0; i < 9; ++i) hyp_H[(size_t)h * 9 + i] = valid ? H[i] : 0.0f;
        if (cnt > bestc) {
            bestc = cnt; besth = h; validb = valid; sgnb = sgn;
            memcpy(Hb, H, sizeof(Hb));
        }
    }
    float G[9];
    h_prep(Hb, k2, sgnb, validb, G);
    int cnt = 0;
    for (int m = 0; m < M; ++m) {
        const int in = h_inlier(G, n1[2 * m], n1[2 * m + 1], S2[2 * m], S2[2 * m + 1]);
        mask[m] = (uint8_t)in;
        cnt += in;
    }
    for (int i = 0; i < 9; ++i) Hout[i] = validb ? Hb[i] : 0.0f;
    norm[0] = cx1; norm[1] = cy1; norm[2] = s1; norm[3] = cx2; norm[4] = cy2; norm[5] = s2;
    *best_h = besth;
    free(n1); free(n2); free(S2);
    return cnt;
}
