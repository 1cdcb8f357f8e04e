// Device camera model shared by the BA and triangulation kernels:
// angle-axis rotation r (3), translation t (3), focal f, radial k1; principal point fixed.
//   pred = f (1 + k1 |p|^2) p + pp,  p = (P0/P2, P1/P2),  P = R(r) X + t.
// Mirrors oracle/sfm_oracle_ba.c (oracle_ba_obs) and oracle/ba_lm.py (_rotmat).
#pragma once
#include <hip/hip_runtime.h>

// Rodrigues; first-order form below |r|^2 = 1e-20 (as the oracle).
__device__ __forceinline__ void rotmat(double r0v, double r1v, double r2v, double (&R)[9]) {
    const double th2 = r0v * r0v + r1v * r1v + r2v * r2v;
    if (th2 > 1e-20) {
        const double th = sqrt(th2);
        double s, c;
        sincos(th, &s, &c);
        const double C = 1.0 - c;
        const double kx = r0v / th, ky = r1v / th, kz = r2v / th;
        R[0] = c + C * kx * kx;      R[1] = C * kx * ky - s * kz; R[2] = C * kx * kz + s * ky;
        R[3] = C * ky * kx + s * kz; R[4] = c + C * ky * ky;      R[5] = C * ky * kz - s * kx;
        R[6] = C * kz * kx - s * ky; R[7] = C * kz * ky + s * kx; R[8] = c + C * kz * kz;
    } else {
        R[0] = 1.0;  R[1] = -r2v; R[2] = r1v;
        R[3] = r2v;  R[4] = 1.0;  R[5] = -r0v;
        R[6] = -r1v; R[7] = r0v;  R[8] = 1.0;
    }
}

// Log map R (row-major) -> angle-axis o, |o| <= pi.  Mirrors oracle/ba_lm.py (_angle_axis).
// cs = (tr R - 1) / 2, w = the axial vector of R - Rᵀ (= 2 sin θ a), sn = |w| / 2, θ = atan2(sn, cs).
//   near π (cs < 0, sn <= 1e-2): a from S = (R + Rᵀ) / 2 - cs I, which is (1 - cs) a aᵀ exactly:
//       its largest-diagonal column j is a_j a with no term in π - θ; sign from w (either sign at
//       θ = π, where w is rounding only);
//   near 0 (sn <= 1e-7):  o = w / 2;
//   otherwise:            o = w θ / (2 sn); its error ε θ / sn stays below 1e-13 on the π side
//                         because of the 1e-2 switch there.
// max |rotmat(o) - R| is a few ε for every θ in [0, π] (tests/test_recon_hp_cpu.py, 1e-12 asserted
// against a 50-digit reference).
__device__ __forceinline__ void log_so3(const double (&R)[9], double& o0, double& o1, double& o2) {
    const double cs = fmin(fmax(0.5 * ((R[0] + R[4] + R[8]) - 1.0), -1.0), 1.0);
    const double w0 = R[7] - R[5], w1 = R[2] - R[6], w2 = R[3] - R[1];
    const double sn = 0.5 * sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double th = atan2(sn, cs);
    if (cs < 0.0 && sn <= 1e-2) {
        const double S0 = R[0] - cs, S4 = R[4] - cs, S8 = R[8] - cs;
        const int j = (S0 >= S4 && S0 >= S8) ? 0 : (S4 >= S8 ? 1 : 2);
        const double s01 = 0.5 * (R[1] + R[3]), s02 = 0.5 * (R[2] + R[6]), s12 = 0.5 * (R[5] + R[7]);
        double a0 = j == 0 ? S0 : (j == 1 ? s01 : s02);  // column j of S
        double a1 = j == 0 ? s01 : (j == 1 ? S4 : s12);
        double a2 = j == 0 ? s02 : (j == 1 ? s12 : S8);
        if (a0 * w0 + a1 * w1 + a2 * w2 < 0.0) { a0 = -a0; a1 = -a1; a2 = -a2; }
        const double k = th / sqrt(a0 * a0 + a1 * a1 + a2 * a2);
        o0 = a0 * k; o1 = a1 * k; o2 = a2 * k;
    } else if (sn > 1e-7) {
        const double k = th / (2.0 * sn);
        o0 = w0 * k; o1 = w1 * k; o2 = w2 * k;
    } else {
        o0 = 0.5 * w0; o1 = 0.5 * w1; o2 = 0.5 * w2;
    }
}
