/*
 * CPU statement of the two-view relative pose spec (TEST INFRASTRUCTURE ONLY; DESIGN.md §4.2b,
 * include/sfmcore.h sfm_two_view_pose_batch).  This file IS the spec: fp64 throughout, only
 * + - * / sqrt in a fixed order (no contraction: -ffp-contract=off), so csrc/two_view_pose.hip
 * must reproduce every output bit for bit.  tests/pose_ref.py is the ctypes front-end.
 * Build: gcc -O3 -march=x86-64-v3 -ffp-contract=off -fno-fast-math -fPIC -shared.
 *
 * Per pair (a, b) with tentative matches, the F batch's mask / inl_count and intr = (f, k1, cx, cy):
 *   coordinates  x_d = (kp - (cx, cy)) / f, undistorted by 10 fixed-point steps from x = x_d of
 *                x = x_d / (1 + k1 |x|^2)  (the triangulation kernel's rule)
 *   fit          N = A^T A over the inliers, rows (x2x x1x, x2x x1y, x2x, x2y x1x, x2y x1y, x2y,
 *                x1x, x1y, 1); each of the 45 sums in fixed_sum order (lane l takes m = l, l+64, ...
 *                ascending, masked-out matches skipped, then the halving tree); E = eigenvector of
 *                N's smallest eigenvalue by cyclic Jacobi (lowest index among equal eigenvalues)
 *   poses        Jacobi on E^T E; v1, v2 by descending eigenvalue, v3 = v1 x v2; u1 = E v1 / |.|,
 *                u2 = (E v2 - (E v2 . u1) u1) / |.|, u3 = u1 x u2; candidates (U W V^T, +u3),
 *                (U W V^T, -u3), (U W^T V^T, +u3), (U W^T V^T, -u3)
 *   scoring      a = R (x1, 1), b = (x2, 1); l1 = (a.b)(b.t) - (a.t)(b.b), l2 = (a.a)(b.t) -
 *                (a.b)(a.t); in front when both > 0; winner = most in front, lowest index on ties
 *   ray angle    s = |a x b|^2 / ((a.a)(b.b)); key = s if a.b >= 0 else 2 - s, rounded to f32;
 *                over the inliers in front under the winner: n_wide = #(key > wide_key) and the
 *                lower median (index (n - 1) / 2 of the ascending keys)
 *   status       0 ok; 1 inl_count < max(min_inliers, 8); 2 degenerate (|E v1| or the
 *                orthogonalised |E v2| not above POSE_TINY); outputs zero unless 0
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define POSE_SWEEPS 30      /* Jacobi sweep cap */
#define POSE_TINY 1e-8      /* vanishing norm of a column of U (E has unit Frobenius norm) */

/* normalised undistorted coordinates of one keypoint */
void pref_undistort(float u, float v, const double intr[4], double x[2]) {
    const double f = intr[0], k1 = intr[1];
    const double xd0 = ((double)u - intr[2]) / f, xd1 = ((double)v - intr[3]) / f;
    double x0 = xd0, x1 = xd1;
    for (int it = 0; it < 10; ++it) {
        const double s = 1.0 + k1 * (x0 * x0 + x1 * x1);
        x0 = xd0 / s;
        x1 = xd1 / s;
    }
    x[0] = x0; x[1] = x1;
}

/* Cyclic Jacobi on a symmetric n x n (n odd; row-major, full storage): A is destroyed, V gets the
 * eigenvectors as columns.  The rotation is triangulate.hip's jacobi4's; the pairs of a sweep come
 * in the round-robin order: round r = 0..n-1 holds the (n-1)/2 disjoint pairs {(r+i) mod n,
 * (r-i) mod n}, i = 1..(n-1)/2 (every pair once per sweep).  A round takes all its (c, s) from
 * the matrix as the round finds it, then applies every column update, then every row update:
 * within each of the two steps the pairs touch disjoint columns / rows, so a round is one
 * parallel step for the kernel and the order inside a step does not matter.  A pair whose
 * off-diagonal element is at most 1e-300 in magnitude gets the identity (c, s) = (1, 0).  Stops
 * after the sweep that leaves the squared off-diagonal at or below 1e-60 of the squared trace (a
 * value test), or at the cap. */
static void jacobi(double* A, double* V, int n) {
    const int h = (n - 1) / 2;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[n * i + j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < POSE_SWEEPS; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) off = off + A[n * p + q] * A[n * p + q];
        double tr = A[0];
        for (int k = 1; k < n; ++k) tr = tr + A[n * k + k];
        if (off <= 1e-60 * tr * tr) break;
        for (int r = 0; r < n; ++r) {
            int P[4], Q[4];
            double cs[4], sn[4];
            for (int i = 0; i < h; ++i) {
                const int a = (r + i + 1) % n, b = (r + n - i - 1) % n;
                const int p = a < b ? a : b, q = a < b ? b : a;
                const double apq = A[n * p + q], app = A[n * p + p], aqq = A[n * q + q];
                double c = 1.0, s = 0.0;
                if (fabs(apq) > 1e-300) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    c = 1.0 / sqrt(tt * tt + 1.0);
                    s = tt * c;
                }
                P[i] = p; Q[i] = q; cs[i] = c; sn[i] = s;
            }
            for (int i = 0; i < h; ++i) {
                const int p = P[i], q = Q[i];
                const double c = cs[i], s = sn[i];
                for (int k = 0; k < n; ++k) { /* A <- A J */
                    const double akp = A[n * k + p], akq = A[n * k + q];
                    A[n * k + p] = c * akp - s * akq;
                    A[n * k + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[n * k + p], vkq = V[n * k + q];
                    V[n * k + p] = c * vkp - s * vkq;
                    V[n * k + q] = s * vkp + c * vkq;
                }
            }
            for (int i = 0; i < h; ++i) {
                const int p = P[i], q = Q[i];
                const double c = cs[i], s = sn[i];
                for (int k = 0; k < n; ++k) { /* A <- J^T A */
                    const double apk = A[n * p + k], aqk = A[n * q + k];
                    A[n * p + k] = c * apk - s * aqk;
                    A[n * q + k] = s * apk + c * aqk;
                }
            }
        }
    }
}

static void row9(const double x1[2], const double x2[2], double r[9]) {
    r[0] = x2[0] * x1[0]; r[1] = x2[0] * x1[1]; r[2] = x2[0];
    r[3] = x2[1] * x1[0]; r[4] = x2[1] * x1[1]; r[5] = x2[1];
    r[6] = x1[0]; r[7] = x1[1]; r[8] = 1.0;
}

/* N = A^T A [9][9] over the masked-in matches m < M; x1 / x2 [M][2] in match order */
void pref_normal_matrix(const double* x1, const double* x2, const uint8_t* mask, int32_t M,
                        double N[81]) {
    double part[64][45];
    memset(part, 0, sizeof(part));
    for (int l = 0; l < 64; ++l)
        for (int m = l; m < M; m += 64) {
            if (!mask[m]) continue;
            double r[9];
            row9(x1 + 2 * m, x2 + 2 * m, r);
            int k = 0;
            for (int i = 0; i < 9; ++i)
                for (int j = i; j < 9; ++j, ++k) part[l][k] = part[l][k] + r[i] * r[j];
        }
    for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l)
            for (int k = 0; k < 45; ++k) part[l][k] = part[l][k] + part[l + off][k];
    int k = 0;
    for (int i = 0; i < 9; ++i)
        for (int j = i; j < 9; ++j, ++k) N[9 * i + j] = N[9 * j + i] = part[0][k];
}

/* E (unit null vector of N, row-major 3x3) -> the two rotations Ra = U W V^T, Rb = U W^T V^T and
 * u3; returns 0 if a column norm of U vanishes */
static int decompose(const double E[9], double Ra[9], double Rb[9], double u3[3]) {
    double G[9], V[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            G[3 * i + j] = (E[i] * E[j] + E[3 + i] * E[3 + j]) + E[6 + i] * E[6 + j];
    jacobi(G, V, 3);
    int i1 = 0;
    for (int k = 1; k < 3; ++k)
        if (G[4 * k] > G[4 * i1]) i1 = k;
    int i2 = (i1 == 0) ? 1 : 0;
    for (int k = i2 + 1; k < 3; ++k)
        if (k != i1 && G[4 * k] > G[4 * i2]) i2 = k;
    double v1[3], v2[3], v3[3], u1[3], u2[3];
    for (int i = 0; i < 3; ++i) { v1[i] = V[3 * i + i1]; v2[i] = V[3 * i + i2]; }
    v3[0] = v1[1] * v2[2] - v1[2] * v2[1];
    v3[1] = v1[2] * v2[0] - v1[0] * v2[2];
    v3[2] = v1[0] * v2[1] - v1[1] * v2[0];
    for (int i = 0; i < 3; ++i) {
        u1[i] = (E[3 * i] * v1[0] + E[3 * i + 1] * v1[1]) + E[3 * i + 2] * v1[2];
        u2[i] = (E[3 * i] * v2[0] + E[3 * i + 1] * v2[1]) + E[3 * i + 2] * v2[2];
    }
    const double n1 = sqrt((u1[0] * u1[0] + u1[1] * u1[1]) + u1[2] * u1[2]);
    if (!(n1 > POSE_TINY)) return 0;
    for (int i = 0; i < 3; ++i) u1[i] = u1[i] / n1;
    const double d = (u2[0] * u1[0] + u2[1] * u1[1]) + u2[2] * u1[2];
    for (int i = 0; i < 3; ++i) u2[i] = u2[i] - d * u1[i];
    const double n2 = sqrt((u2[0] * u2[0] + u2[1] * u2[1]) + u2[2] * u2[2]);
    if (!(n2 > POSE_TINY)) return 0;
    for (int i = 0; i < 3; ++i) u2[i] = u2[i] / n2;
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            Ra[3 * i + j] = (u2[i] * v1[j] - u1[i] * v2[j]) + u3[i] * v3[j];
            Rb[3 * i + j] = (u1[i] * v2[j] - u2[i] * v1[j]) + u3[i] * v3[j];
        }
    return 1;
}

/* one inlier under (R, t): in front (1/0) and the f32 ray-angle key (depends on R only) */
static int score(const double R[9], const double t[3], const double x1[2], const double x2[2],
                 float* key) {
    double a[3];
    for (int i = 0; i < 3; ++i) a[i] = (R[3 * i] * x1[0] + R[3 * i + 1] * x1[1]) + R[3 * i + 2];
    const double b0 = x2[0], b1 = x2[1], b2 = 1.0;
    const double aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    const double bb = (b0 * b0 + b1 * b1) + b2 * b2;
    const double ab = (a[0] * b0 + a[1] * b1) + a[2] * b2;
    const double at = (a[0] * t[0] + a[1] * t[1]) + a[2] * t[2];
    const double bt = (b0 * t[0] + b1 * t[1]) + b2 * t[2];
    const double l1 = ab * bt - at * bb;
    const double l2 = aa * bt - ab * at;
    const double c0 = a[1] * b2 - a[2] * b1, c1 = a[2] * b0 - a[0] * b2, c2 = a[0] * b1 - a[1] * b0;
    const double s = ((c0 * c0 + c1 * c1) + c2 * c2) / (aa * bb);
    *key = (float)(ab >= 0.0 ? s : 2.0 - s);
    return (l1 > 0.0 && l2 > 0.0) ? 1 : 0;
}

static int cmp_u32(const void* a, const void* b) {
    const uint32_t x = *(const uint32_t*)a, y = *(const uint32_t*)b;
    return x < y ? -1 : (x > y ? 1 : 0);
}

/* One pair.  x1 / x2 [M][2]: undistorted coordinates in match order.  Outputs E, R [9], t [3],
 * stat [8] = {status, best, n_front[4], n_wide, inliers used}, median_key. */
void pref_pose(const double* x1, const double* x2, const uint8_t* mask, int32_t M,
               int32_t inl_count, int32_t min_inliers, float wide_key, double E[9], double R[9],
               double t[3], int32_t stat[8], float* median_key) {
    memset(E, 0, 9 * sizeof(double));
    memset(R, 0, 9 * sizeof(double));
    memset(t, 0, 3 * sizeof(double));
    memset(stat, 0, 8 * sizeof(int32_t));
    *median_key = 0.0f;
    if (inl_count < (min_inliers > 8 ? min_inliers : 8)) { stat[0] = 1; return; }
    double N[81], V[81], e[9], Rc[2][9], u3[3];
    pref_normal_matrix(x1, x2, mask, M, N);
    jacobi(N, V, 9);
    int kmin = 0;
    for (int k = 1; k < 9; ++k)
        if (N[10 * k] < N[10 * kmin]) kmin = k;
    for (int i = 0; i < 9; ++i) e[i] = V[9 * i + kmin];
    if (!decompose(e, Rc[0], Rc[1], u3)) { stat[0] = 2; return; }
    int n_inl = 0, nf[4] = {0, 0, 0, 0};
    for (int m = 0; m < M; ++m) {
        if (!mask[m]) continue;
        ++n_inl;
        for (int c = 0; c < 4; ++c) {
            const double tc[3] = {(c & 1) ? -u3[0] : u3[0], (c & 1) ? -u3[1] : u3[1],
                                  (c & 1) ? -u3[2] : u3[2]};
            float key;
            nf[c] += score(Rc[c >> 1], tc, x1 + 2 * m, x2 + 2 * m, &key);
        }
    }
    int best = 0;
    for (int c = 1; c < 4; ++c)
        if (nf[c] > nf[best]) best = c;
    const double tb[3] = {(best & 1) ? -u3[0] : u3[0], (best & 1) ? -u3[1] : u3[1],
                          (best & 1) ? -u3[2] : u3[2]};
    uint32_t* keys = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(M > 0 ? M : 1));
    int n = 0, n_wide = 0;
    for (int m = 0; m < M; ++m) {
        if (!mask[m]) continue;
        float key;
        if (!score(Rc[best >> 1], tb, x1 + 2 * m, x2 + 2 * m, &key)) continue;
        n_wide += (key > wide_key) ? 1 : 0;
        memcpy(&keys[n++], &key, 4);  /* keys are >= 0: the bit pattern orders like the value */
    }
    if (n > 0) {
        qsort(keys, (size_t)n, sizeof(uint32_t), cmp_u32);
        memcpy(median_key, &keys[(n - 1) / 2], 4);
    }
    free(keys);
    memcpy(E, e, sizeof(e));
    memcpy(R, Rc[best >> 1], 9 * sizeof(double));
    memcpy(t, tb, sizeof(tb));
    stat[1] = best;
    for (int c = 0; c < 4; ++c) stat[2 + c] = nf[c];
    stat[6] = n_wide;
    stat[7] = n_inl;
}

/* The candidates of a fitted E: Ra, Rb [9], u3 [3] (candidate c = (c >> 1 ? Rb : Ra, c & 1 ? -u3 :
 * u3)); returns 0 where pref_pose reports status 2 */
int32_t pref_candidates(const double E[9], double Ra[9], double Rb[9], double u3[3]) {
    return decompose(E, Ra, Rb, u3);
}

static int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

/* The batch, with the arguments of sfm_two_view_pose_batch (host arrays).  Image ids, match counts
 * and keypoint indices are clamped to their arrays, as the kernels clamp them. */
void pref_pose_batch(const float* kps, int32_t n_img, int32_t k_max, const int32_t* pairs,
                     int32_t P, const int32_t* match_count, const int32_t* matches,
                     const uint8_t* mask, const int32_t* inl_count, const double* intr,
                     int32_t min_inliers, float wide_key, double* E, double* R, double* t,
                     int32_t* stat, float* median_key) {
    double* x1 = (double*)malloc(sizeof(double) * 2 * (size_t)(k_max > 0 ? k_max : 1));
    double* x2 = (double*)malloc(sizeof(double) * 2 * (size_t)(k_max > 0 ? k_max : 1));
    for (int p = 0; p < P; ++p) {
        const int a = clampi(pairs[2 * p], n_img - 1), b = clampi(pairs[2 * p + 1], n_img - 1);
        const int M = clampi(match_count[p], k_max);
        const int32_t* mt = matches + (size_t)p * k_max * 2;
        for (int m = 0; m < M; ++m) {
            const float* ka = kps + ((size_t)a * k_max + clampi(mt[2 * m], k_max - 1)) * 2;
            const float* kb = kps + ((size_t)b * k_max + clampi(mt[2 * m + 1], k_max - 1)) * 2;
            pref_undistort(ka[0], ka[1], intr + 4 * a, x1 + 2 * m);
            pref_undistort(kb[0], kb[1], intr + 4 * b, x2 + 2 * m);
        }
        pref_pose(x1, x2, mask + (size_t)p * k_max, M, inl_count[p], min_inliers, wide_key,
                  E + 9 * p, R + 9 * p, t + 3 * p, stat + 8 * p, median_key + p);
    }
    free(x1); free(x2);
}
