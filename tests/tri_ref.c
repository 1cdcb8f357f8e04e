/* CPU statement of the robust triangulation spec (csrc/triangulate_robust.hip header; TEST
 * INFRASTRUCTURE ONLY).  fp64, the operations in the order written, built without FMA contraction
 * (tests/tri_ref.py).  The GPU results equal these bit for bit, except stats[1], whose acos is
 * libm's here.
 *
 * The spec starts from the per-camera table [n_cam][20] = R (9, row-major), t (3), C = -R^T t (3),
 * f, k1, pp (2), 0.  triref_cam_table builds it with libm's sin / cos; the GPU tests pass the
 * library's own table (sfm_triangulate_cam_table) instead, because the two sincos differ in the
 * last bit.
 *
 * Hypothesis h of a track with n observations, integer rule:
 *   n (n - 1) / 2 <= max_hyp: the h-th pair (i < j) in lexicographic order,
 *       i = 0; while (h >= n - 1 - i) { h -= n - 1 - i; ++i; }  j = i + 1 + h;
 *   otherwise: r = Philox4x32-10(counter = (h, 3, pt_id, 0x54524931), key = (seed & 0xffffffff,
 *       seed >> 32)); a = (r[0] * n) >> 32; b = (r[1] * (n - 1)) >> 32 (64-bit products);
 *       if (b >= a) ++b;  (i, j) = (min(a, b), max(a, b)).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define CAMW 20
#define UNDISTORT_ITERS 10
#define JACOBI_SWEEPS 10

static void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                          uint32_t k1, uint32_t out[4]) {
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

int triref_n_hyp(int n, int max_hyp) {
    const long long np = (long long)n * (n - 1) / 2;
    return np <= (long long)max_hyp ? (int)np : max_hyp;
}

void triref_pair(int h, int n, int max_hyp, uint64_t seed, uint32_t id, int* ij) {
    const long long np = (long long)n * (n - 1) / 2;
    if (np <= (long long)max_hyp) {
        int rem = h, i = 0;
        while (rem >= n - 1 - i) { rem -= n - 1 - i; ++i; }
        ij[0] = i; ij[1] = i + 1 + rem;
    } else {
        uint32_t r[4];
        philox4x32_10((uint32_t)h, 3u, id, 0x54524931u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
        const uint32_t a = (uint32_t)(((uint64_t)r[0] * (uint32_t)n) >> 32);
        uint32_t b = (uint32_t)(((uint64_t)r[1] * (uint32_t)(n - 1)) >> 32);
        if (b >= a) ++b;
        ij[0] = (int)(a < b ? a : b);
        ij[1] = (int)(a < b ? b : a);
    }
}

void triref_cam_table(int n_cam, const double* cams, const double* pp, double* tab) {
    for (int c = 0; c < n_cam; ++c) {
        const double* cam = cams + 8 * (size_t)c;
        double* o = tab + CAMW * (size_t)c;
        double R[9];
        const double r0 = cam[0], r1 = cam[1], r2 = cam[2];
        const double th2 = r0 * r0 + r1 * r1 + r2 * r2;
        if (th2 > 1e-20) {
            const double th = sqrt(th2), s = sin(th), cs = cos(th), C = 1.0 - cs;
            const double kx = r0 / th, ky = r1 / th, kz = r2 / th;
            R[0] = cs + C * kx * kx;     R[1] = C * kx * ky - s * kz; R[2] = C * kx * kz + s * ky;
            R[3] = C * ky * kx + s * kz; R[4] = cs + C * ky * ky;     R[5] = C * ky * kz - s * kx;
            R[6] = C * kz * kx - s * ky; R[7] = C * kz * ky + s * kx; R[8] = cs + C * kz * kz;
        } else {
            R[0] = 1.0; R[1] = -r2; R[2] = r1;
            R[3] = r2;  R[4] = 1.0; R[5] = -r0;
            R[6] = -r1; R[7] = r0;  R[8] = 1.0;
        }
        for (int k = 0; k < 9; ++k) o[k] = R[k];
        o[9] = cam[3]; o[10] = cam[4]; o[11] = cam[5];
        for (int j = 0; j < 3; ++j)
            o[12 + j] = -(R[j] * cam[3] + R[3 + j] * cam[4] + R[6 + j] * cam[5]);
        o[15] = cam[6]; o[16] = cam[7];
        o[17] = pp[2 * (size_t)c]; o[18] = pp[2 * (size_t)c + 1];
        o[19] = 0.0;
    }
}

static void jacobi4(double* A, double* V) {
    for (int k = 0; k < 16; ++k) V[k] = (k % 5 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) off += A[4 * p + q] * A[4 * p + q];
        const double tr = A[0] + A[5] + A[10] + A[15];
        if (off <= 1e-60 * tr * tr) break;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[4 * p + q];
                if (fabs(apq) <= 1e-300) continue;
                const double app = A[4 * p + p], aqq = A[4 * q + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double tt =
                    (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
                for (int k = 0; k < 4; ++k) {
                    const double akp = A[4 * k + p], akq = A[4 * k + q];
                    A[4 * k + p] = c * akp - s * akq;
                    A[4 * k + q] = s * akp + c * akq;
                }
                for (int k = 0; k < 4; ++k) {
                    const double apk = A[4 * p + k], aqk = A[4 * q + k];
                    A[4 * p + k] = c * apk - s * aqk;
                    A[4 * q + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 4; ++k) {
                    const double vkp = V[4 * k + p], vkq = V[4 * k + q];
                    V[4 * k + p] = c * vkp - s * vkq;
                    V[4 * k + q] = s * vkp + c * vkq;
                }
            }
    }
}

/* One observation: table row o, pixel, undistorted x, world ray d. */
typedef struct {
    const double* o;
    double u, v, x0, x1, d[3];
} view_t;

static void make_view(const double* tab, int c, double u, double v, view_t* w) {
    const double* o = tab + CAMW * (size_t)c;
    const double f = o[15], k1 = o[16];
    const double xd0 = (u - o[17]) / f, xd1 = (v - o[18]) / f;
    double x0 = xd0, x1 = xd1;
    for (int it = 0; it < UNDISTORT_ITERS; ++it) {
        const double s = 1.0 + k1 * (x0 * x0 + x1 * x1);
        x0 = xd0 / s;
        x1 = xd1 / s;
    }
    w->o = o; w->u = u; w->v = v; w->x0 = x0; w->x1 = x1;
    for (int m = 0; m < 3; ++m) w->d[m] = o[m] * x0 + o[3 + m] * x1 + o[6 + m];
}

static int conforms(const view_t* w, const double* X, double thr2, double* P2o, double* e2o) {
    const double* r = w->o;
    const double P0 = r[0] * X[0] + r[1] * X[1] + r[2] * X[2] + r[9];
    const double P1 = r[3] * X[0] + r[4] * X[1] + r[5] * X[2] + r[10];
    const double P2 = r[6] * X[0] + r[7] * X[1] + r[8] * X[2] + r[11];
    const double q0 = P0 / P2, q1 = P1 / P2;
    const double g = 1.0 + r[16] * (q0 * q0 + q1 * q1);
    const double e0 = r[15] * g * q0 + r[17] - w->u;
    const double e1 = r[15] * g * q1 + r[18] - w->v;
    const double e2 = e0 * e0 + e1 * e1;
    *P2o = P2; *e2o = e2;
    return P2 > 0.0 && e2 < thr2;
}

static double dot3(const double* a, const double* b) {
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

static int two_view_point(const view_t* vi, const view_t* vj, double max_cos2, double* X) {
    const double *a = vi->d, *b = vj->d, *Ci = vi->o + 12, *Cj = vj->o + 12;
    double w[3];
    for (int m = 0; m < 3; ++m) w[m] = Cj[m] - Ci[m];
    const double c = dot3(a, b), aa = dot3(a, a), bb = dot3(b, b);
    if (!(c > 0.0 && c * c < max_cos2 * (aa * bb))) return 0;
    const double aw = dot3(a, w), bw = dot3(b, w);
    const double det = aa * bb - c * c;
    const double s = (bb * aw - c * bw) / det, t = (c * aw - aa * bw) / det;
    if (!(s > 0.0 && t > 0.0)) return 0;
    for (int m = 0; m < 3; ++m) X[m] = 0.5 * ((Ci[m] + s * a[m]) + (Cj[m] + t * b[m]));
    return 1;
}

static void walk(const view_t* vw, int n, const double* X, double thr2, uint8_t* mask, int* cnt,
                 double* err, double* dmin) {
    *cnt = 0; *err = 0.0; *dmin = 1e300;
    for (int k = 0; k < n; ++k) {
        double P2, e2;
        const int ok = conforms(vw + k, X, thr2, &P2, &e2);
        if (mask) mask[k] = (uint8_t)ok;
        if (ok) {
            ++*cnt;
            *err += sqrt(e2);
            *dmin = fmin(*dmin, P2);
        }
    }
}

void triref_run(const double* tab, int n_pt, const int32_t* pt_ptr, const int32_t* cam_idx,
                const double* uv, const int32_t* pt_id, double thr, double max_cos2, int max_hyp,
                uint64_t seed, double* out_pts, double* out_stats, uint8_t* out_mask,
                int32_t* out_info) {
    const double thr2 = thr * thr;
    for (int p = 0; p < n_pt; ++p) {
        const int o0 = pt_ptr[p], n = pt_ptr[p + 1] - o0;
        double* Xo = out_pts + 3 * (size_t)p;
        double* S = out_stats + 4 * (size_t)p;
        int32_t* I = out_info + 2 * (size_t)p;
        Xo[0] = Xo[1] = Xo[2] = 0.0;
        S[0] = S[1] = S[2] = 0.0;
        I[0] = 0; I[1] = -1;
        for (int k = 0; k < n; ++k) out_mask[o0 + k] = 0;
        if (n < 2) { S[3] = 1.0; continue; }
        view_t* vw = (view_t*)malloc(sizeof(view_t) * (size_t)n);
        for (int k = 0; k < n; ++k)
            make_view(tab, cam_idx[o0 + k], uv[2 * (size_t)(o0 + k)], uv[2 * (size_t)(o0 + k) + 1],
                      vw + k);
        const int n_hyp = triref_n_hyp(n, max_hyp);
        int hw = -1, cw = 0;
        double Xw[3] = {0.0, 0.0, 0.0};
        for (int h = 0; h < n_hyp; ++h) {
            int ij[2];
            double X[3];
            triref_pair(h, n, max_hyp, seed, (uint32_t)pt_id[p], ij);
            if (!two_view_point(vw + ij[0], vw + ij[1], max_cos2, X)) continue;
            int cnt = 0;
            for (int k = 0; k < n; ++k) {
                double P2, e2;
                cnt += conforms(vw + k, X, thr2, &P2, &e2);
            }
            if (cnt >= 2 && cnt > cw) { cw = cnt; hw = h; memcpy(Xw, X, sizeof X); }
        }
        if (hw < 0) { S[3] = 4.0; free(vw); continue; }
        /* refit over the winner's consensus set */
        double M[16], V[16];
        for (int k = 0; k < 16; ++k) M[k] = 0.0;
        for (int k = 0; k < n; ++k) {
            double P2, e2;
            if (!conforms(vw + k, Xw, thr2, &P2, &e2)) continue;
            const double* R = vw[k].o;
            double r0[4], r1[4];
            for (int m = 0; m < 3; ++m) {
                r0[m] = vw[k].x0 * R[6 + m] - R[m];
                r1[m] = vw[k].x1 * R[6 + m] - R[3 + m];
            }
            r0[3] = vw[k].x0 * R[11] - R[9];
            r1[3] = vw[k].x1 * R[11] - R[10];
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) M[4 * i + j] += r0[i] * r0[j] + r1[i] * r1[j];
        }
        jacobi4(M, V);
        int kmin = 0;
        for (int k = 1; k < 4; ++k)
            if (M[5 * k] < M[5 * kmin]) kmin = k;
        const double h0 = V[kmin], h1 = V[4 + kmin], h2 = V[8 + kmin], h3 = V[12 + kmin];
        const double nh = sqrt(h0 * h0 + h1 * h1 + h2 * h2);
        double Xf[3], ef, df;
        int cf, kept = 0;
        if (fabs(h3) > 1e-12 * nh) {
            double Xr[3] = {h0 / h3, h1 / h3, h2 / h3};
            walk(vw, n, Xr, thr2, NULL, &cf, &ef, &df);
            if (cf >= cw) { kept = 1; memcpy(Xf, Xr, sizeof Xf); }
        }
        if (!kept) memcpy(Xf, Xw, sizeof Xf);
        walk(vw, n, Xf, thr2, out_mask + o0, &cf, &ef, &df);
        double cmax = 1.0;
        for (int i = 0; i < n; ++i) {
            if (!out_mask[o0 + i]) continue;
            const double* Ci = vw[i].o + 12;
            const double a0 = Xf[0] - Ci[0], a1 = Xf[1] - Ci[1], a2 = Xf[2] - Ci[2];
            const double na = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
            for (int j = i + 1; j < n; ++j) {
                if (!out_mask[o0 + j]) continue;
                const double* Cj = vw[j].o + 12;
                const double b0 = Xf[0] - Cj[0], b1 = Xf[1] - Cj[1], b2 = Xf[2] - Cj[2];
                const double nb = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
                cmax = fmin(cmax, (a0 * b0 + a1 * b1 + a2 * b2) / (na * nb));
            }
        }
        Xo[0] = Xf[0]; Xo[1] = Xf[1]; Xo[2] = Xf[2];
        S[0] = ef / (double)cf;
        S[1] = acos(fmax(-1.0, fmin(1.0, cmax))) * (180.0 / 3.14159265358979323846);
        S[2] = df;
        S[3] = 0.0;
        I[0] = cf; I[1] = hw;
        free(vw);
    }
}
