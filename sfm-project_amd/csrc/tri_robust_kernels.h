// The kernels of the robust triangulation (spec and kernel notes: the header of
// triangulate_robust.hip), shared by sfm_triangulate_robust and sfm_triangulate_multi: one
// definition, so every round of the recursion executes the operations of the single call.
#pragma once
#include "tri_common.h"

namespace tri_robust {
namespace {  // internal linkage: every translation unit gets its own copy

using namespace tri;

// View record: 0-8 R, 9-11 t, 12-14 C, 15 f, 16 k1, 17-18 pp, 19-20 uv, 21-22 x, 23-25 d.  The
// long-track kernel reuses the fields that have done their work (see its tail).
constexpr int RECW = 26;
constexpr int N_BIN = 4;

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Hypothesis h -> view pair (i < j).
__device__ __forceinline__ void pair_of(int h, int n, bool exhaustive, uint64_t seed, uint32_t id,
                                        int& i, int& j) {
    if (exhaustive) {
        int rem = h;
        i = 0;
        while (rem >= n - 1 - i) { rem -= n - 1 - i; ++i; }
        j = i + 1 + rem;
    } else {
        uint32_t r[4];
        philox4x32_10((uint32_t)h, 3u, id, 0x54524931u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
        const uint32_t a = __umulhi(r[0], (uint32_t)n);
        uint32_t b = __umulhi(r[1], (uint32_t)(n - 1));
        if (b >= a) ++b;
        i = (int)(a < b ? a : b);
        j = (int)(a < b ? b : a);
    }
}

// The camera part of a record (fields 0-20) from table row o and the pixel.
__device__ __forceinline__ void build_cam(const double* __restrict__ o, double u, double v,
                                          double* r) {
#pragma unroll
    for (int k = 0; k < 19; ++k) r[k] = o[k];
    r[19] = u; r[20] = v;
}
// Fields 21-25: undistorted coordinates and the world ray.
__device__ __forceinline__ void build_ray(const double* __restrict__ o, double u, double v,
                                          double* r) {
    double x0, x1;
    undistort(o, u, v, x0, x1);
    r[21] = x0; r[22] = x1;
#pragma unroll
    for (int m = 0; m < 3; ++m) r[23 + m] = o[m] * x0 + o[3 + m] * x1 + o[6 + m];
}

// A track as its group sees it: the staged records and where the rest comes from.
struct Track {
    const double* lds;   // CAP records
    const double* tab;
    const int32_t* cam;  // cam_idx + o0
    const double* uv;    // uv + 2 o0
    int n;
};

template <int CAP, bool RAY>
__device__ __forceinline__ void load_rec(const Track& T, int k, double (&r)[RECW]) {
    if (k < CAP) {
        const double* s = T.lds + RECW * k;
#pragma unroll
        for (int q = 0; q < (RAY ? RECW : 21); ++q) r[q] = s[q];
    } else {
        const double* o = T.tab + CAMW * (size_t)T.cam[k];
        const double u = T.uv[2 * (size_t)k], v = T.uv[2 * (size_t)k + 1];
        build_cam(o, u, v, r);
        if (RAY) build_ray(o, u, v, r);
    }
}

__device__ __forceinline__ bool conforms(const double (&r)[RECW], const double (&X)[3], double thr2,
                                         double& P2, double& e2) {
    const double P0 = r[0] * X[0] + r[1] * X[1] + r[2] * X[2] + r[9];
    const double P1 = r[3] * X[0] + r[4] * X[1] + r[5] * X[2] + r[10];
    P2 = r[6] * X[0] + r[7] * X[1] + r[8] * X[2] + r[11];
    const double q0 = P0 / P2, q1 = P1 / P2;
    const double g = 1.0 + r[16] * (q0 * q0 + q1 * q1);
    const double e0 = r[15] * g * q0 + r[17] - r[19];
    const double e1 = r[15] * g * q1 + r[18] - r[20];
    e2 = e0 * e0 + e1 * e1;
    return P2 > 0.0 && e2 < thr2;
}

__device__ __forceinline__ double dot3(const double* a, const double* b) {
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// Step 3 for hypothesis h.
template <int CAP>
__device__ __forceinline__ bool two_view_point(const Track& T, int h, bool exhaustive,
                                               uint64_t seed, uint32_t id, double max_cos2,
                                               double (&X)[3]) {
    int i, j;
    pair_of(h, T.n, exhaustive, seed, id, i, j);
    double ri[RECW], rj[RECW];
    load_rec<CAP, true>(T, i, ri);
    load_rec<CAP, true>(T, j, rj);
    const double* a = ri + 23;
    const double* b = rj + 23;
    double w[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) w[m] = rj[12 + m] - ri[12 + m];
    const double c = dot3(a, b), aa = dot3(a, a), bb = dot3(b, b);
    if (!(c > 0.0 && c * c < max_cos2 * (aa * bb))) return false;
    const double aw = dot3(a, w), bw = dot3(b, w);
    const double det = aa * bb - c * c;
    const double s = (bb * aw - c * bw) / det, t = (c * aw - aa * bw) / det;
    if (!(s > 0.0 && t > 0.0)) return false;
#pragma unroll
    for (int m = 0; m < 3; ++m) X[m] = 0.5 * ((ri[12 + m] + s * a[m]) + (rj[12 + m] + t * b[m]));
    return true;
}

// All n observations under X, every lane the same walk: count, Σ sqrt(e2) and min depth of the
// conforming ones, in CSR order.
template <int CAP>
__device__ __forceinline__ void walk(const Track& T, const double (&X)[3], double thr2, int& cnt,
                                     double& err, double& dmin) {
    cnt = 0; err = 0.0; dmin = 1e300;
    for (int k = 0; k < T.n; ++k) {
        double r[RECW], P2, e2;
        load_rec<CAP, false>(T, k, r);
        if (conforms(r, X, thr2, P2, e2)) {
            ++cnt;
            err += sqrt(e2);
            dmin = fmin(dmin, P2);
        }
    }
}

__device__ __forceinline__ double sel4(const double (&v)[4], int i) {
    return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3]));
}

// FUSED: the group also refits and writes the track's outputs (long tracks).  Otherwise it stops
// at the winner, {count, h} in out_info, and tri_finish_kernel does the rest a thread per track.
template <int G, int CAP, bool FUSED>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void tri_robust_kernel(
    const int32_t* __restrict__ bin_count, const int32_t* __restrict__ list,
    const int32_t* __restrict__ pt_ptr, const int32_t* __restrict__ cam_idx,
    const double* __restrict__ uv, const int32_t* __restrict__ pt_id,
    const double* __restrict__ tab, double thr2, double max_cos2, int max_hyp, uint64_t seed,
    double* __restrict__ out_pts, double* __restrict__ out_stats, uint8_t* __restrict__ out_mask,
    int32_t* __restrict__ out_info) {
    constexpr int TPW = 64 / G;            // tracks per wave
    __shared__ double lds[TPW * CAP * RECW];
    const int lane = threadIdx.x, g = lane / G, gl = lane % G;
    double* L = lds + (size_t)g * CAP * RECW;
    const int n_list = *bin_count;
    for (int base = blockIdx.x * TPW; base < n_list; base += gridDim.x * TPW) {
        const bool act = base + g < n_list;
        int p = 0, o0 = 0, n = 0;
        if (act) {
            p = list[base + g];
            o0 = pt_ptr[p];
            n = pt_ptr[p + 1] - o0;
        }
        Track T{L, tab, cam_idx + o0, uv + 2 * (size_t)o0, n};
        __syncthreads();   // the previous track's records are no longer read
        for (int k = gl; k < n && k < CAP; k += G) {
            const double* o = tab + CAMW * (size_t)T.cam[k];
            const double u = T.uv[2 * (size_t)k], v = T.uv[2 * (size_t)k + 1];
            double r[RECW];
            build_cam(o, u, v, r);
            build_ray(o, u, v, r);
#pragma unroll
            for (int q = 0; q < RECW; ++q) L[RECW * k + q] = r[q];
        }
        __syncthreads();
        const long long n_pairs = (long long)n * (n - 1) / 2;
        const bool exhaustive = n_pairs <= (long long)max_hyp;
        const int n_hyp = exhaustive ? (int)n_pairs : max_hyp;
        const uint32_t id = act ? (uint32_t)pt_id[p] : 0u;

        // ---- a lane per hypothesis, passes of G
        unsigned long long best = 0ull;
        for (int h0 = 0; h0 < n_hyp; h0 += G) {
            const int h = h0 + gl;
            double X[3] = {0.0, 0.0, 0.0};
            bool valid = h < n_hyp;
            if (valid) valid = two_view_point<CAP>(T, h, exhaustive, seed, id, max_cos2, X);
            int cnt = 0;
            for (int k = 0; k < n; ++k) {
                double r[RECW], P2, e2;
                load_rec<CAP, false>(T, k, r);
                cnt += conforms(r, X, thr2, P2, e2) ? 1 : 0;
            }
            if (valid && cnt >= 2) {
                const unsigned long long key =
                    ((unsigned long long)(uint32_t)cnt << 32) | (uint32_t)~(uint32_t)h;
                best = key > best ? key : best;
            }
        }
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off, 64);
            best = o > best ? o : best;
        }
        const bool found = best != 0ull;
        const int hw = found ? (int)~(uint32_t)best : -1;
        const int cw = (int)(best >> 32);
        if constexpr (!FUSED) {
            if (act && gl == 0) {
                out_info[2 * (size_t)p] = cw;
                out_info[2 * (size_t)p + 1] = hw;
            }
            continue;
        }

        // ---- long tracks (one per wave: found is uniform).  Per-observation work is split over
        // the lanes and left in the record's dead fields (23 flag, 24 sqrt(e2), 25 depth); sums
        // that have an order are then formed by every lane from those, in CSR order.
        static_assert(!FUSED || G == 64, "the fused tail takes one track per wave");
        const int n_lds = n < CAP ? n : CAP;
        auto par_eval = [&](const double (&X)[3]) {
            __syncthreads();
            for (int k = gl; k < n_lds; k += G) {
                double r[RECW], P2, e2;
                load_rec<CAP, false>(T, k, r);
                const bool ok = conforms(r, X, thr2, P2, e2);
                L[RECW * k + 23] = ok ? 1.0 : 0.0;
                L[RECW * k + 24] = sqrt(e2);
                L[RECW * k + 25] = P2;
            }
            __syncthreads();
        };
        auto seq_sum = [&](const double (&X)[3], int& cnt, double& err, double& dmin) {
            cnt = 0; err = 0.0; dmin = 1e300;
            for (int k = 0; k < n; ++k) {
                bool ok;
                double se, P2;
                if (k < CAP) {
                    ok = L[RECW * k + 23] != 0.0;
                    se = L[RECW * k + 24];
                    P2 = L[RECW * k + 25];
                } else {
                    double r[RECW], e2;
                    load_rec<CAP, false>(T, k, r);
                    ok = conforms(r, X, thr2, P2, e2);
                    se = sqrt(e2);
                }
                if (ok) {
                    ++cnt;
                    err += se;
                    dmin = fmin(dmin, P2);
                }
            }
        };
        double Xf[3] = {0.0, 0.0, 0.0}, Xw[3] = {0.0, 0.0, 0.0};
        int cf = 0;
        double ef = 0.0, df = 0.0;
        if (found) two_view_point<CAP>(T, hw, exhaustive, seed, id, max_cos2, Xw);
        par_eval(Xw);   // the rays (23-25) are dead from here on
        bool kept = false;
        if (found) {
            double acc = 0.0;   // entry gl & 15 of M
            const int ei = (gl & 15) >> 2, ej = gl & 3;
            for (int k = 0; k < n; ++k) {
                double r[RECW];
                if (k < CAP) {
                    if (L[RECW * k + 23] == 0.0) continue;
                    load_rec<CAP, false>(T, k, r);
                    r[21] = L[RECW * k + 21];
                    r[22] = L[RECW * k + 22];
                } else {
                    double P2, e2;
                    load_rec<CAP, true>(T, k, r);
                    if (!conforms(r, Xw, thr2, P2, e2)) continue;
                }
                double r0[4], r1[4];
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    r0[m] = r[21] * r[6 + m] - r[m];
                    r1[m] = r[22] * r[6 + m] - r[3 + m];
                }
                r0[3] = r[21] * r[11] - r[9];
                r1[3] = r[22] * r[11] - r[10];
                acc += sel4(r0, ei) * sel4(r0, ej) + sel4(r1, ei) * sel4(r1, ej);
            }
            double M[16], V[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) M[e] = __shfl(acc, e, 64);
            jacobi4(M, V);
            int kmin = 0;
            for (int k = 1; k < 4; ++k)
                if (M[5 * k] < M[5 * kmin]) kmin = k;
            double hv[4];
#pragma unroll
            for (int m = 0; m < 4; ++m)
                hv[m] = kmin == 0 ? V[4 * m] : (kmin == 1 ? V[4 * m + 1]
                                                : (kmin == 2 ? V[4 * m + 2] : V[4 * m + 3]));
            const double nh = sqrt(hv[0] * hv[0] + hv[1] * hv[1] + hv[2] * hv[2]);
            kept = fabs(hv[3]) > 1e-12 * nh;
            if (kept) {
                Xf[0] = hv[0] / hv[3]; Xf[1] = hv[1] / hv[3]; Xf[2] = hv[2] / hv[3];
            }
        }
        if (kept) {
            par_eval(Xf);
            seq_sum(Xf, cf, ef, df);
            kept = cf >= cw;
        }
        if (found && !kept) {
            Xf[0] = Xw[0]; Xf[1] = Xw[1]; Xf[2] = Xw[2];
            par_eval(Xf);
            seq_sum(Xf, cf, ef, df);
        }

        // ---- the mask, and the rays of the kept point: 21, 22, 24 the ray X - C, 25 its length
        __syncthreads();
        for (int k = gl; k < n; k += G) {
            double r[RECW], P2, e2;
            load_rec<CAP, false>(T, k, r);
            const bool ok = found && (k < CAP ? L[RECW * k + 23] != 0.0
                                              : conforms(r, Xf, thr2, P2, e2));
            out_mask[(size_t)o0 + k] = ok ? 1 : 0;
            if (k < CAP) {
                const double a0 = Xf[0] - r[12], a1 = Xf[1] - r[13], a2 = Xf[2] - r[14];
                double* s = L + RECW * k;
                s[21] = a0; s[22] = a1; s[24] = a2;
                s[25] = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
            }
        }
        __syncthreads();
        double cmax = 1.0;
        if (found) {
            for (int i = gl; i < n; i += G) {
                double a[5];   // flag, ray, length
                auto ray = [&](int k, double (&o)[5]) {
                    if (k < CAP) {
                        const double* s = L + RECW * k;
                        o[0] = s[23]; o[1] = s[21]; o[2] = s[22]; o[3] = s[24]; o[4] = s[25];
                    } else {
                        double r[RECW], P2, e2;
                        load_rec<CAP, false>(T, k, r);
                        o[0] = conforms(r, Xf, thr2, P2, e2) ? 1.0 : 0.0;
                        o[1] = Xf[0] - r[12]; o[2] = Xf[1] - r[13]; o[3] = Xf[2] - r[14];
                        o[4] = sqrt(o[1] * o[1] + o[2] * o[2] + o[3] * o[3]);
                    }
                };
                ray(i, a);
                if (a[0] == 0.0) continue;
                for (int j = i + 1; j < n; ++j) {
                    double b[5];
                    ray(j, b);
                    if (b[0] == 0.0) continue;
                    cmax = fmin(cmax, (a[1] * b[1] + a[2] * b[2] + a[3] * b[3]) / (a[4] * b[4]));
                }
            }
        }
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) cmax = fmin(cmax, __shfl_xor(cmax, off, 64));
        if (act && gl == 0) {
            double* X = out_pts + 3 * (size_t)p;
            double* S = out_stats + 4 * (size_t)p;
            int32_t* I = out_info + 2 * (size_t)p;
            X[0] = Xf[0]; X[1] = Xf[1]; X[2] = Xf[2];
            if (found) {
                S[0] = ef / (double)cf;
                S[1] = acos(fmax(-1.0, fmin(1.0, cmax))) * (180.0 / 3.14159265358979323846);
                S[2] = df;
                S[3] = 0.0;
            } else {
                S[0] = 0.0; S[1] = 0.0; S[2] = 0.0; S[3] = 4.0;
            }
            I[0] = cf;
            I[1] = hw;
        }
    }
}

// Short tracks after the winner search, thread per track as sfm_triangulate (a group would run the
// same Jacobi on every lane): the winner's point again, the refit, rescoring, mask and stats, all
// from the camera table.  Its tracks are those of the first three lists.
__global__ __launch_bounds__(256) void tri_finish_kernel(
    int n_pt, const int32_t* __restrict__ counts, const int32_t* __restrict__ lists,
    const int32_t* __restrict__ pt_ptr, const int32_t* __restrict__ cam_idx,
    const double* __restrict__ uv, const int32_t* __restrict__ pt_id,
    const double* __restrict__ tab, double thr2, double max_cos2, int max_hyp, uint64_t seed,
    double* __restrict__ out_pts, double* __restrict__ out_stats, uint8_t* out_mask,
    int32_t* out_info) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    int b = 0;
    while (b < N_BIN - 1 && t >= counts[b]) t -= counts[b++];
    if (b == N_BIN - 1) return;
    const int p = lists[(size_t)b * n_pt + t];
    const int o0 = pt_ptr[p], n = pt_ptr[p + 1] - o0;
    const Track T{nullptr, tab, cam_idx + o0, uv + 2 * (size_t)o0, n};
    double* X = out_pts + 3 * (size_t)p;
    double* S = out_stats + 4 * (size_t)p;
    uint8_t* mk = out_mask + o0;
    const int hw = out_info[2 * (size_t)p + 1], cw = out_info[2 * (size_t)p];
    if (hw < 0) {
        X[0] = X[1] = X[2] = 0.0;
        S[0] = 0.0; S[1] = 0.0; S[2] = 0.0; S[3] = 4.0;
        for (int k = 0; k < n; ++k) mk[k] = 0;
        out_info[2 * (size_t)p] = 0;
        return;
    }
    const long long n_pairs = (long long)n * (n - 1) / 2;
    double Xw[3], Xf[3];
    two_view_point<0>(T, hw, n_pairs <= (long long)max_hyp, seed, (uint32_t)pt_id[p], max_cos2, Xw);
    double M[16], V[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) M[k] = 0.0;
    for (int k = 0; k < n; ++k) {
        double r[RECW], P2, e2;
        load_rec<0, true>(T, k, r);
        if (!conforms(r, Xw, thr2, P2, e2)) continue;
        double r0[4], r1[4];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            r0[m] = r[21] * r[6 + m] - r[m];
            r1[m] = r[22] * r[6 + m] - r[3 + m];
        }
        r0[3] = r[21] * r[11] - r[9];
        r1[3] = r[22] * r[11] - r[10];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) M[4 * i + j] += r0[i] * r0[j] + r1[i] * r1[j];
    }
    jacobi4(M, V);
    int kmin = 0;
    for (int k = 1; k < 4; ++k)
        if (M[5 * k] < M[5 * kmin]) kmin = k;
    const double h0 = V[kmin], h1 = V[4 + kmin], h2 = V[8 + kmin], h3 = V[12 + kmin];
    const double nh = sqrt(h0 * h0 + h1 * h1 + h2 * h2);
    int cf = 0;
    double ef = 0.0, df = 0.0;
    bool kept = false;
    if (fabs(h3) > 1e-12 * nh) {
        const double Xr[3] = {h0 / h3, h1 / h3, h2 / h3};
        walk<0>(T, Xr, thr2, cf, ef, df);
        if (cf >= cw) {
            kept = true;
            Xf[0] = Xr[0]; Xf[1] = Xr[1]; Xf[2] = Xr[2];
        }
    }
    if (!kept) {
        Xf[0] = Xw[0]; Xf[1] = Xw[1]; Xf[2] = Xw[2];
        walk<0>(T, Xf, thr2, cf, ef, df);
    }
    for (int k = 0; k < n; ++k) {
        double r[RECW], P2, e2;
        load_rec<0, false>(T, k, r);
        mk[k] = conforms(r, Xf, thr2, P2, e2) ? 1 : 0;
    }
    double cmax = 1.0;
    for (int i = 0; i < n; ++i) {   // the flags just written by this thread
        if (!mk[i]) continue;
        const double* ci = tab + CAMW * (size_t)T.cam[i] + 12;
        const double a0 = Xf[0] - ci[0], a1 = Xf[1] - ci[1], a2 = Xf[2] - ci[2];
        const double na = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
        for (int j = i + 1; j < n; ++j) {
            if (!mk[j]) continue;
            const double* cj = tab + CAMW * (size_t)T.cam[j] + 12;
            const double b0 = Xf[0] - cj[0], b1 = Xf[1] - cj[1], b2 = Xf[2] - cj[2];
            const double nb = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
            cmax = fmin(cmax, (a0 * b0 + a1 * b1 + a2 * b2) / (na * nb));
        }
    }
    X[0] = Xf[0]; X[1] = Xf[1]; X[2] = Xf[2];
    S[0] = ef / (double)cf;
    S[1] = acos(fmax(-1.0, fmin(1.0, cmax))) * (180.0 / 3.14159265358979323846);
    S[2] = df;
    S[3] = 0.0;
    out_info[2 * (size_t)p] = cf;
}

// Tracks of more than this many observations go to the long-track list whatever their
// hypothesis count (a small max_hyp): their refit and statistics want a group, not a thread.
constexpr int SHORT_MAX_OBS = 16;

// Thread per track: status 1 written here, every other track appended to the list of its bin.
// List positions: one atomic per block and bin (100 k single atomics on one counter took 1.1 ms);
// inside the block the positions follow the thread order.  n_pt is the capacity (the grid and the
// stride of the lists); n_live, where given, is the device-side number of tracks below it.
__global__ __launch_bounds__(256) void tri_bin(int n_pt, const int32_t* __restrict__ n_live,
                                               const int32_t* __restrict__ pt_ptr,
                                               int max_hyp, int32_t* __restrict__ counts,
                                               int32_t* __restrict__ lists,
                                               double* __restrict__ out_pts,
                                               double* __restrict__ out_stats,
                                               uint8_t* __restrict__ out_mask,
                                               int32_t* __restrict__ out_info) {
    __shared__ int32_t wave_cnt[4][N_BIN], bin_base[N_BIN];
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int b = -1;
    if (p < (n_live ? *n_live : n_pt)) {
        const int o0 = pt_ptr[p], n = pt_ptr[p + 1] - o0;
        if (n < 2) {
            double* X = out_pts + 3 * (size_t)p;
            double* S = out_stats + 4 * (size_t)p;
            X[0] = X[1] = X[2] = 0.0;
            S[0] = 0.0; S[1] = 0.0; S[2] = 0.0; S[3] = 1.0;
            if (n == 1) out_mask[o0] = 0;
            out_info[2 * (size_t)p] = 0;
            out_info[2 * (size_t)p + 1] = -1;
        } else {
            const long long n_pairs = (long long)n * (n - 1) / 2;
            const int n_hyp = n_pairs <= (long long)max_hyp ? (int)n_pairs : max_hyp;
            b = n > SHORT_MAX_OBS ? 3
                                  : (n_hyp <= 8 ? 0 : (n_hyp <= 16 ? 1 : (n_hyp <= 32 ? 2 : 3)));
        }
    }
    int before = 0;   // threads of this wave in the same bin before this one
#pragma unroll
    for (int q = 0; q < N_BIN; ++q) {
        const unsigned long long m = __ballot(b == q);
        if (b == q) before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wave][q] = __popcll(m);
    }
    __syncthreads();
    if (threadIdx.x < N_BIN) {
        const int q = threadIdx.x;
        const int tot = wave_cnt[0][q] + wave_cnt[1][q] + wave_cnt[2][q] + wave_cnt[3][q];
        bin_base[q] = tot ? atomicAdd(&counts[q], tot) : 0;
    }
    __syncthreads();
    if (b >= 0) {
        int pos = bin_base[b] + before;
        for (int w = 0; w < wave; ++w) pos += wave_cnt[w][b];
        lists[(size_t)b * n_pt + pos] = p;
    }
}

template <int G, int CAP, bool FUSED>
void launch_bin(sfm_ctx* ctx, int b, int waves_per_cu, const int32_t* counts, const int32_t* lists,
                int32_t n_pt, const int32_t* pt_ptr, const int32_t* cam_idx, const double* uv,
                const int32_t* pt_id, const double* tab, double thr2, double max_cos2, int max_hyp,
                uint64_t seed, double* out_pts, double* out_stats, uint8_t* out_mask,
                int32_t* out_info) {
    constexpr int TPW = 64 / G;
    const long long need = ((long long)n_pt + TPW - 1) / TPW;
    const long long cap = (long long)ctx->n_cu * waves_per_cu;
    const int grid = (int)(need < cap ? need : cap);
    hipLaunchKernelGGL((tri_robust_kernel<G, CAP, FUSED>), dim3(grid), dim3(64), 0, ctx->stream,
                       counts + b, lists + (size_t)b * n_pt, pt_ptr, cam_idx, uv, pt_id, tab, thr2,
                       max_cos2, max_hyp, seed, out_pts, out_stats, out_mask, out_info);
}

// Everything after the camera table, enqueued on the context's stream: the bins (counts: N_BIN
// zeroed counters, lists: N_BIN * n_pt entries), the searches and the finish.  n_pt sizes the
// grids; with n_live (device) only that many tracks exist and the rest of every grid returns at
// once.
inline void enqueue(sfm_ctx* ctx, int32_t n_pt, const int32_t* n_live, int32_t* counts,
                    int32_t* lists, const int32_t* pt_ptr, const int32_t* cam_idx, const double* uv,
                    const int32_t* pt_id, const double* tab, double thr2, double max_cos2,
                    int max_hyp, uint64_t seed, double* out_pts, double* out_stats,
                    uint8_t* out_mask, int32_t* out_info) {
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(tri_bin, dim3((n_pt + 255) / 256), dim3(256), 0, st, n_pt, n_live, pt_ptr,
                       max_hyp, counts, lists, out_pts, out_stats, out_mask, out_info);
#define TRI_BIN_LAUNCH(G, CAP, FUSED, B, WPC)                                                     \
    launch_bin<G, CAP, FUSED>(ctx, B, WPC, counts, lists, n_pt, pt_ptr, cam_idx, uv, pt_id, tab,  \
                              thr2, max_cos2, max_hyp, seed, out_pts, out_stats, out_mask,        \
                              out_info)
    TRI_BIN_LAUNCH(8, 4, false, 0, 16);
    TRI_BIN_LAUNCH(16, 6, false, 1, 16);
    TRI_BIN_LAUNCH(32, 8, false, 2, 16);
    hipLaunchKernelGGL(tri_finish_kernel, dim3((n_pt + 255) / 256), dim3(256), 0, st, n_pt, counts,
                       lists, pt_ptr, cam_idx, uv, pt_id, tab, thr2, max_cos2, max_hyp, seed,
                       out_pts, out_stats, out_mask, out_info);
    TRI_BIN_LAUNCH(64, 128, true, 3, 6);
#undef TRI_BIN_LAUNCH
}

}  // namespace
}  // namespace tri_robust
