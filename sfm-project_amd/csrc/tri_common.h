// Shared by the triangulation kernels (triangulate.hip, tri_robust_kernels.h): the per-camera
// table, the fixed-point undistortion and the 4x4 Jacobi eigen-solver of the multi-view DLT.  One
// definition, so both kernels execute the same operations in the same order.
#pragma once
#include "camera_model.h"
#include "sfm_internal.h"

namespace tri {
namespace {  // internal linkage: every translation unit gets its own copy

constexpr int UNDISTORT_ITERS = 10;
constexpr int JACOBI_SWEEPS = 10;

// Per-camera table (once per launch): R (9), t (3), centre C = -Rᵀ t (3), f, k1, pp (2) = 20.
constexpr int CAMW = 20;

__global__ __launch_bounds__(256) void tri_cam_setup(int n_cam, const double* __restrict__ cams,
                                                     const double* __restrict__ pp,
                                                     double* __restrict__ tab) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cam) return;
    const double* cam = cams + 8 * (size_t)c;
    double R[9];
    rotmat(cam[0], cam[1], cam[2], R);
    double* o = tab + CAMW * (size_t)c;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = R[k];
    o[9] = cam[3]; o[10] = cam[4]; o[11] = cam[5];
#pragma unroll
    for (int j = 0; j < 3; ++j) o[12 + j] = -(R[j] * cam[3] + R[3 + j] * cam[4] + R[6 + j] * cam[5]);
    o[15] = cam[6]; o[16] = cam[7];
    o[17] = pp[2 * (size_t)c]; o[18] = pp[2 * (size_t)c + 1];
    o[19] = 0.0;
}

// Undistorted normalised coordinates of pixel (u, v) under table row o.
__device__ __forceinline__ void undistort(const double* __restrict__ o, double u, double v,
                                          double& x0o, double& x1o) {
    const double f = o[15], k1 = o[16];
    const double xd0 = (u - o[17]) / f, xd1 = (v - o[18]) / f;
    double x0 = xd0, x1 = xd1;
    for (int it = 0; it < UNDISTORT_ITERS; ++it) {
        const double s = 1.0 + k1 * (x0 * x0 + x1 * x1);
        x0 = xd0 / s;
        x1 = xd1 / s;
    }
    x0o = x0; x1o = x1;
}

struct View {
    double R[9], t[3];
    double x0, x1;  // undistorted normalised coordinates
};

__device__ __forceinline__ void load_view(const double* __restrict__ tab, int c, double u,
                                          double v, View& w) {
    const double* o = tab + CAMW * (size_t)c;
#pragma unroll
    for (int k = 0; k < 9; ++k) w.R[k] = o[k];
    w.t[0] = o[9]; w.t[1] = o[10]; w.t[2] = o[11];
    undistort(o, u, v, w.x0, w.x1);
}

// Cyclic Jacobi on a symmetric 4x4: A is destroyed, V gets the eigenvectors (columns).  Stops
// after the sweep that leaves the off-diagonal below 1e-30 of the trace (a value test: the same
// inputs stop at the same sweep).
__device__ void jacobi4(double (&A)[16], double (&V)[16]) {
#pragma unroll
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
                const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
                for (int k = 0; k < 4; ++k) {  // A <- Jᵀ A J
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

}  // namespace
}  // namespace tri
