// Batched two-view relative pose: the stage after "F / H" of two-view
// verification (papers/schoenberger2016sfm.pdf §4.1-4.2).  From the F batch's inlier mask and the
// per-image intrinsics: a linear essential fit over the inliers, the four (R, t) decompositions,
// the cheirality vote and the triangulation (ray) angle of the inliers in front.
//
// The spec is tests/pose_ref.c: fp64 throughout, only + - * / sqrt in a fixed order, built like
// this file with -ffp-contract=off, so every output equals the CPU's bit for bit.
//
// Three kernels per call:
//   pose_table  one thread per keypoint: normalised, undistorted coordinates (the triangulation
//               kernel's 10 fixed-point steps) into an [n_img][k_max][2] f64 table, once per call
//               rather than once per pair.
//   pose_fit    one WAVE per pair.  Lane l accumulates the 45 unique sums of N = A^T A over the
//               masked-in matches m = l, l+64, ... ascending (four gathers in flight), then the
//               halving tree (wave_fixed_sum): the spec's summation order.  Cyclic Jacobi on the
//               9x9 in LDS in the spec's round-robin order: the four disjoint rotations of a round
//               and, within each, the column / row / eigenvector element updates are independent
//               and go to one lane each (jacobi_wave), so the bits are the serial loop's.  The
//               same routine on E^T E (3x3), then U, V, the two rotations and u3 in registers.
//   pose_score  one 256-thread block per pair.  Sweep 1 gathers the inliers from the table and
//               counts the four candidates (the -u3 candidates are the +u3 ones with both depth
//               numerators negated, exactly), then picks the winner.  Sweep 2 writes the winner's
//               f32 ray-angle keys of the inliers in front to LDS and counts the wide ones; the
//               lower median is an exact radix select (4 passes of 8 bits) on the keys' bit
//               patterns, which order like the values because the keys are non-negative.
// All counts are integers, so nothing depends on the block width, the batch or the pair order.
#include "ransac_common.h"

namespace {

constexpr int POSE_SWEEPS = 30;     // Jacobi sweep cap (pose_ref.c)
constexpr double POSE_TINY = 1e-8;  // vanishing norm of a column of U
constexpr int SCORE_T = 256;
constexpr unsigned KEY_NONE = 0xFFFFFFFFu;  // LDS slot of a match that is not an inlier in front

__global__ __launch_bounds__(256) void pose_table_kernel(const float* __restrict__ kps,
                                                         const double* __restrict__ intr,
                                                         int k_max, int n_total,
                                                         double* __restrict__ tab) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_total) return;
    const double* o = intr + 4 * (size_t)(i / k_max);
    const V2<float> kp = *(const V2<float>*)(kps + 2 * (size_t)i);
    const double f = o[0], k1 = o[1];
    const double xd0 = ((double)kp.x - o[2]) / f, xd1 = ((double)kp.y - o[3]) / f;
    double x0 = xd0, x1 = xd1;
    for (int it = 0; it < 10; ++it) {
        const double s = 1.0 + k1 * (x0 * x0 + x1 * x1);
        x0 = xd0 / s;
        x1 = xd1 / s;
    }
    V2<double> w;
    w.x = x0; w.y = x1;
    *(V2<double>*)(tab + 2 * (size_t)i) = w;
}

// a wave-uniform double as such for the compiler (branches on it become scalar branches)
__device__ __forceinline__ double uniform(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Cyclic Jacobi on the symmetric n x n A in LDS (row-major, n odd, n <= 9), by one wave: A is
// destroyed, V gets the eigenvectors as columns (pose_ref.c jacobi, op for op).  A sweep is n
// rounds of (n - 1) / 2 disjoint pairs (round-robin order).  Lane j * n + k serves pair j of the
// round and row / column k: it derives the pair's (c, s) from the matrix as the round finds it
// (every lane of a pair computes the same bits), updates row k of A's and V's columns (p, q),
// and after the barrier column k of A's rows (p, q).  The lanes of one step write disjoint
// elements, so a round of up to four rotations costs one rotation's dependent chain.
__device__ void jacobi_wave(double* A, double* V, int n, int lane) {
    const int h = (n - 1) / 2;
    const int j = lane / n, k = lane - j * n;
    const bool act = lane < h * n;
    for (int i = lane; i < n * n; i += 64) V[i] = (i / n == i % n) ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < POSE_SWEEPS; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) off = off + A[n * p + q] * A[n * p + q];
        double tr = A[0];
        for (int i = 1; i < n; ++i) tr = tr + A[n * i + i];
        off = uniform(off);
        tr = uniform(tr);
        if (off <= 1e-60 * tr * tr) break;
        for (int r = 0; r < n; ++r) {
            // pair j of round r: {(r + j + 1) mod n, (r - j - 1) mod n}; idle lanes shadow pair 0
            const int jj = act ? j : 0;
            int a = r + jj + 1, b = r + n - jj - 1;
            a = a >= n ? a - n : a;
            b = b >= n ? b - n : b;
            const int p = min(a, b), q = max(a, b);
            const double apq = A[n * p + q], app = A[n * p + p], aqq = A[n * q + q];
            const double theta = (aqq - app) / (2.0 * apq);
            const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double cr = 1.0 / sqrt(tt * tt + 1.0), sr = tt * cr;
            const bool rot = fabs(apq) > 1e-300;
            const double c = rot ? cr : 1.0, s = rot ? sr : 0.0;
            if (act) {
                const double akp = A[n * k + p], akq = A[n * k + q];
                A[n * k + p] = c * akp - s * akq;
                A[n * k + q] = s * akp + c * akq;
                const double vkp = V[n * k + p], vkq = V[n * k + q];
                V[n * k + p] = c * vkp - s * vkq;
                V[n * k + q] = s * vkp + c * vkq;
            }
            __syncthreads();
            if (act) {
                const double apk = A[n * p + k], aqk = A[n * q + k];
                A[n * p + k] = c * apk - s * aqk;
                A[n * q + k] = s * apk + c * aqk;
            }
            __syncthreads();
        }
    }
    __syncthreads();
}

__device__ __forceinline__ double dot3(const double a[3], const double b[3]) {
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
__device__ __forceinline__ void cross3(const double a[3], const double b[3], double c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

constexpr int CANDW = 21;  // per pair in the workspace: Ra (9), Rb (9), u3 (3)

__global__ __launch_bounds__(64) void pose_fit_kernel(
    int n_img, int k_max, const int32_t* __restrict__ pairs, const int32_t* __restrict__ match_count,
    const int32_t* __restrict__ matches, const uint8_t* __restrict__ mask,
    const int32_t* __restrict__ inl_count, const double* __restrict__ tab, int min_inliers,
    double* __restrict__ out_E, double* __restrict__ cand, int32_t* __restrict__ out_stat) {
    __shared__ double A[81], V[81], Es[9];
    const int p = blockIdx.x, lane = threadIdx.x;
    double* E = out_E + 9 * (size_t)p;
    int32_t* st = out_stat + 8 * (size_t)p;
    if (inl_count[p] < max(min_inliers, 8)) {  // block-uniform
        if (lane < 9) E[lane] = 0.0;
        if (lane < 8) st[lane] = lane == 0 ? 1 : 0;
        return;
    }
    // ids and counts are clamped to the arrays (a no-op on valid input: no read goes out of bounds)
    const int a = clampi(pairs[2 * p], n_img - 1), b = clampi(pairs[2 * p + 1], n_img - 1);
    const int M = clampi(match_count[p], k_max);
    const int32_t* mt = matches + (size_t)p * k_max * 2;
    const uint8_t* mk = mask + (size_t)p * k_max;
    const double* ta = tab + (size_t)a * k_max * 2;
    const double* tb = tab + (size_t)b * k_max * 2;

    double acc[45];
#pragma unroll
    for (int k = 0; k < 45; ++k) acc[k] = 0.0;
    for (int m0 = lane; m0 < M; m0 += 256) {
        bool on[4];
        int2 id[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int m = m0 + 64 * t;
            on[t] = m < M && mk[m < M ? m : 0] != 0;
            id[t] = on[t] ? *(const int2*)(mt + 2 * m) : make_int2(0, 0);
        }
        V2<double> u[4], v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            u[t] = *(const V2<double>*)(ta + 2 * (size_t)clampi(id[t].x, k_max - 1));
            v[t] = *(const V2<double>*)(tb + 2 * (size_t)clampi(id[t].y, k_max - 1));
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (!on[t]) continue;
            const double r[9] = {v[t].x * u[t].x, v[t].x * u[t].y, v[t].x,
                                 v[t].y * u[t].x, v[t].y * u[t].y, v[t].y,
                                 u[t].x, u[t].y, 1.0};
            int k = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i)
#pragma unroll
                for (int j = i; j < 9; ++j, ++k) acc[k] = acc[k] + r[i] * r[j];
        }
    }
    {
        int k = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int j = i; j < 9; ++j, ++k) {
                const double s = wave_fixed_sum(acc[k]);
                if (lane == 0) { A[9 * i + j] = s; A[9 * j + i] = s; }
            }
    }
    __syncthreads();
    jacobi_wave(A, V, 9, lane);
    int kmin = 0;
    for (int k = 1; k < 9; ++k)
        if (A[10 * k] < A[10 * kmin]) kmin = k;
    if (lane < 9) Es[lane] = V[9 * lane + kmin];
    __syncthreads();
    double e[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) e[i] = Es[i];
    __syncthreads();  // A is reused below
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                A[3 * i + j] = (e[i] * e[j] + e[3 + i] * e[3 + j]) + e[6 + i] * e[6 + j];
    }
    __syncthreads();
    jacobi_wave(A, V, 3, lane);
    int i1 = 0;
    for (int k = 1; k < 3; ++k)
        if (A[4 * k] > A[4 * i1]) i1 = k;
    int i2 = (i1 == 0) ? 1 : 0;
    for (int k = i2 + 1; k < 3; ++k)
        if (k != i1 && A[4 * k] > A[4 * i2]) i2 = k;
    double v1[3], v2[3], v3[3], u1[3], u2[3], u3[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { v1[i] = V[3 * i + i1]; v2[i] = V[3 * i + i2]; }
    cross3(v1, v2, v3);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        u1[i] = (e[3 * i] * v1[0] + e[3 * i + 1] * v1[1]) + e[3 * i + 2] * v1[2];
        u2[i] = (e[3 * i] * v2[0] + e[3 * i + 1] * v2[1]) + e[3 * i + 2] * v2[2];
    }
    bool ok = true;
    const double n1 = sqrt(dot3(u1, u1));
    ok = ok && (n1 > POSE_TINY);
#pragma unroll
    for (int i = 0; i < 3; ++i) u1[i] = u1[i] / n1;
    const double d = dot3(u2, u1);
#pragma unroll
    for (int i = 0; i < 3; ++i) u2[i] = u2[i] - d * u1[i];
    const double n2 = sqrt(dot3(u2, u2));
    ok = ok && (n2 > POSE_TINY);
#pragma unroll
    for (int i = 0; i < 3; ++i) u2[i] = u2[i] / n2;
    cross3(u1, u2, u3);
    if (lane == 0) {
        double* c = cand + CANDW * (size_t)p;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                c[3 * i + j] = (u2[i] * v1[j] - u1[i] * v2[j]) + u3[i] * v3[j];
                c[9 + 3 * i + j] = (u1[i] * v2[j] - u2[i] * v1[j]) + u3[i] * v3[j];
            }
#pragma unroll
        for (int i = 0; i < 3; ++i) c[18 + i] = u3[i];
#pragma unroll
        for (int i = 0; i < 9; ++i) E[i] = ok ? e[i] : 0.0;
        st[0] = ok ? 0 : 2;
    }
}

// one inlier under R and +t: the depth numerators' signs and the f32 ray-angle key (pose_ref.c
// score).  Returns +1 when both numerators are > 0, -1 when both are < 0 (in front under -t), else 0.
__device__ __forceinline__ int score1(const double R[9], const double t[3], double x1x, double x1y,
                                      double b0, double b1, float& key) {
    double a[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) a[i] = (R[3 * i] * x1x + R[3 * i + 1] * x1y) + R[3 * i + 2];
    const double b2 = 1.0;
    const double aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    const double bb = (b0 * b0 + b1 * b1) + b2 * b2;
    const double ab = (a[0] * b0 + a[1] * b1) + a[2] * b2;
    const double at = (a[0] * t[0] + a[1] * t[1]) + a[2] * t[2];
    const double bt = (b0 * t[0] + b1 * t[1]) + b2 * t[2];
    const double l1 = ab * bt - at * bb;
    const double l2 = aa * bt - ab * at;
    const double c0 = a[1] * b2 - a[2] * b1, c1 = a[2] * b0 - a[0] * b2, c2 = a[0] * b1 - a[1] * b0;
    const double s = ((c0 * c0 + c1 * c1) + c2 * c2) / (aa * bb);
    key = (float)(ab >= 0.0 ? s : 2.0 - s);
    return (l1 > 0.0 && l2 > 0.0) ? 1 : ((l1 < 0.0 && l2 < 0.0) ? -1 : 0);
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(SCORE_T) void pose_score_kernel(
    int n_img, int k_max, const int32_t* __restrict__ pairs, const int32_t* __restrict__ match_count,
    const int32_t* __restrict__ matches, const uint8_t* __restrict__ mask,
    const double* __restrict__ tab, const double* __restrict__ cand, float wide_key,
    double* __restrict__ out_R, double* __restrict__ out_t, int32_t* __restrict__ out_stat,
    float* __restrict__ out_median) {
    extern __shared__ unsigned keys[];  // [k_max]
    __shared__ int cnt[6];              // n_front[4], inliers, n_wide
    __shared__ unsigned hist[256], wtot[4], sel[2];
    const int p = blockIdx.x, tid = threadIdx.x;
    int32_t* st = out_stat + 8 * (size_t)p;
    if (st[0] != 0) {  // written by pose_fit (stream order); block-uniform
        if (tid < 9) out_R[9 * (size_t)p + tid] = 0.0;
        if (tid < 3) out_t[3 * (size_t)p + tid] = 0.0;
        if (tid >= 1 && tid < 8) st[tid] = 0;
        if (tid == 0) out_median[p] = 0.0f;
        return;
    }
    // ids and counts are clamped to the arrays (a no-op on valid input: no read goes out of bounds)
    const int a = clampi(pairs[2 * p], n_img - 1), b = clampi(pairs[2 * p + 1], n_img - 1);
    const int M = clampi(match_count[p], k_max);
    const int2* mt = (const int2*)(matches + (size_t)p * k_max * 2);
    const uint8_t* mk = mask + (size_t)p * k_max;
    const V2<double>* ta = (const V2<double>*)(tab + (size_t)a * k_max * 2);
    const V2<double>* tb = (const V2<double>*)(tab + (size_t)b * k_max * 2);
    double Ra[9], Rb[9], u3[3];
    {
        const double* c = cand + CANDW * (size_t)p;
#pragma unroll
        for (int i = 0; i < 9; ++i) { Ra[i] = c[i]; Rb[i] = c[9 + i]; }
#pragma unroll
        for (int i = 0; i < 3; ++i) u3[i] = c[18 + i];
    }
    if (tid < 6) cnt[tid] = 0;
    __syncthreads();

    // sweep 1: the four candidates' counts
    int nf0 = 0, nf1 = 0, nf2 = 0, nf3 = 0, ni = 0;
    for (int m = tid; m < M; m += SCORE_T) {
        if (!mk[m]) continue;
        const int2 id = mt[m];
        const V2<double> x1 = ta[clampi(id.x, k_max - 1)], x2 = tb[clampi(id.y, k_max - 1)];
        float key;
        const int sa = score1(Ra, u3, x1.x, x1.y, x2.x, x2.y, key);
        const int sb = score1(Rb, u3, x1.x, x1.y, x2.x, x2.y, key);
        nf0 += sa > 0; nf1 += sa < 0; nf2 += sb > 0; nf3 += sb < 0;
        ++ni;
    }
    nf0 = wave_sum_int(nf0); nf1 = wave_sum_int(nf1); nf2 = wave_sum_int(nf2);
    nf3 = wave_sum_int(nf3); ni = wave_sum_int(ni);
    if ((tid & 63) == 0) {
        atomicAdd(&cnt[0], nf0); atomicAdd(&cnt[1], nf1); atomicAdd(&cnt[2], nf2);
        atomicAdd(&cnt[3], nf3); atomicAdd(&cnt[4], ni);
    }
    __syncthreads();
    int best = 0;
#pragma unroll
    for (int c = 1; c < 4; ++c)
        if (cnt[c] > cnt[best]) best = c;
    const int n = cnt[best];
    double Rw[9], tw[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rw[i] = (best >> 1) ? Rb[i] : Ra[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) tw[i] = (best & 1) ? -u3[i] : u3[i];

    // sweep 2: the winner's keys of the inliers in front
    int nw = 0;
    for (int m = tid; m < M; m += SCORE_T) {
        unsigned kb = KEY_NONE;
        if (mk[m]) {
            const int2 id = mt[m];
            const V2<double> x1 = ta[clampi(id.x, k_max - 1)], x2 = tb[clampi(id.y, k_max - 1)];
            float key;
            if (score1(Rw, tw, x1.x, x1.y, x2.x, x2.y, key) > 0) {
                kb = __float_as_uint(key);
                nw += key > wide_key;
            }
        }
        keys[m] = kb;
    }
    nw = wave_sum_int(nw);
    if ((tid & 63) == 0) atomicAdd(&cnt[5], nw);

    // lower median: the element of rank (n - 1) / 2, most significant byte first
    unsigned prefix = 0, kk = n > 0 ? (unsigned)(n - 1) / 2u : 0u;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        if (tid == 0) { sel[0] = prefix; sel[1] = kk; }
        __syncthreads();  // also: keys and cnt[5] of sweep 2 are complete
        const unsigned himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (int m = tid; m < M; m += SCORE_T) {
            const unsigned kb = keys[m];
            if (kb != KEY_NONE && (kb & himask) == prefix) atomicAdd(&hist[(kb >> shift) & 255u], 1u);
        }
        __syncthreads();
        const unsigned h = hist[tid];
        unsigned inc = h;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned o = __shfl_up(inc, off, 64);
            if ((tid & 63) >= off) inc += o;
        }
        if ((tid & 63) == 63) wtot[tid >> 6] = inc;
        __syncthreads();
        unsigned excl = inc - h;
        for (int w = 0; w < (tid >> 6); ++w) excl += wtot[w];
        if (h > 0 && kk >= excl && kk < excl + h) {  // at most one thread
            sel[0] = prefix | ((unsigned)tid << shift);
            sel[1] = kk - excl;
        }
        __syncthreads();
        prefix = sel[0];
        kk = sel[1];
        __syncthreads();
    }
    {   // the winner's pose from the workspace copy (no per-lane index into registers)
        const double* c = cand + CANDW * (size_t)p;
        if (tid < 9) out_R[9 * (size_t)p + tid] = c[(best >> 1) * 9 + tid];
        if (tid < 3) out_t[3 * (size_t)p + tid] = (best & 1) ? -c[18 + tid] : c[18 + tid];
    }
    if (tid == 0) {
        st[1] = best;
        st[2] = cnt[0]; st[3] = cnt[1]; st[4] = cnt[2]; st[5] = cnt[3];
        st[6] = cnt[5];
        st[7] = cnt[4];
        out_median[p] = n > 0 ? __uint_as_float(prefix) : 0.0f;
    }
}

}  // namespace

extern "C" int sfm_two_view_pose_batch(sfm_ctx* ctx, const float* kps, int32_t n_img,
                                       int32_t k_max, const int32_t* pairs, int32_t n_pairs,
                                       const int32_t* match_count, const int32_t* matches,
                                       const uint8_t* mask, const int32_t* inl_count,
                                       const double* intr, const sfm_two_view_pose_params* prm,
                                       double* out_E, double* out_R, double* out_t,
                                       int32_t* out_stat, float* out_median_key) {
    SFM_REQUIRE(ctx && prm, "sfm_two_view_pose_batch: ctx/prm is NULL");
    SFM_REQUIRE(prm->struct_size >= (int32_t)sizeof(sfm_two_view_pose_params),
                "sfm_two_view_pose_batch: prm->struct_size is smaller than the struct");
    SFM_REQUIRE(n_pairs >= 0 && n_img >= 0 && k_max >= 0, "sfm_two_view_pose_batch: negative size");
    if (n_pairs == 0) return SFM_OK;
    SFM_REQUIRE(kps && pairs && match_count && matches && mask && inl_count && intr,
                "sfm_two_view_pose_batch: NULL array");
    SFM_REQUIRE(out_E && out_R && out_t && out_stat && out_median_key,
                "sfm_two_view_pose_batch: NULL output");
    SFM_REQUIRE(n_img > 0 && k_max > 0, "sfm_two_view_pose_batch: no keypoints");
    SFM_REQUIRE(k_max <= 8192, "sfm_two_view_pose_batch: k_max > 8192 not supported");
    SFM_REQUIRE((int64_t)n_img * k_max < (int64_t)1 << 30,
                "sfm_two_view_pose_batch: n_img * k_max too large");
    SFM_REQUIRE(prm->wide_key >= 0.0f, "sfm_two_view_pose_batch: wide_key must be >= 0");
    SFM_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int n_total = n_img * k_max;
    const size_t tabb = sfm::align_up((size_t)n_total * 2 * sizeof(double), 256);
    const size_t candb = sfm::align_up((size_t)n_pairs * CANDW * sizeof(double), 256);
    char* ws = (char*)sfm::workspace(ctx, tabb + candb);
    if (!ws) return SFM_ERR_NOMEM;
    double* tab = (double*)ws;
    double* cand = (double*)(ws + tabb);
    hipLaunchKernelGGL(pose_table_kernel, dim3((n_total + 255) / 256), dim3(256), 0, st, kps, intr,
                       k_max, n_total, tab);
    SFM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pose_fit_kernel, dim3(n_pairs), dim3(64), 0, st, n_img, k_max, pairs,
                       match_count, matches, mask, inl_count, tab, prm->min_inliers, out_E, cand,
                       out_stat);
    SFM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pose_score_kernel, dim3(n_pairs), dim3(SCORE_T),
                       (size_t)k_max * sizeof(unsigned), st, n_img, k_max, pairs, match_count,
                       matches, mask, tab, cand, prm->wide_key, out_R, out_t, out_stat,
                       out_median_key);
    SFM_HIP_CHECK(hipGetLastError());
    return SFM_OK;
}
