// Image retrieval for pair selection: nearest vocabulary word of every
// descriptor, per-image term frequencies, and the top-k images by weighted histogram intersection.
// The assignment here is for L2 / 128-byte descriptors (retrieval_hamming.hip has the one for
// binary descriptors; the other kernels work on word ids and serve both); everything is integer
// and exact, so every output is a function of the inputs alone (no dependence on block or atomic
// order).
//
// sfm_vocab_assign — the hot kernel, K1's exact i8 formulation with the vocabulary as the train
// side.  With x' = x ^ 0x80 (u8 -> i8):  d^2(x, w) = |x'|^2 + |w'|^2 - 2 x'.w', so the nearest
// word maximises vr = 2 x'.w' - |w'|^2.  The dot products run on v_mfma_i32_32x32x32_i8 (exact
// int32) and the word index rides in the low 7 bits of the row key:
//     Kr = 256 dot + crow_j = 128 vr + (127 - j mod 128)
// A plain max over a group of 128 words therefore yields (largest vr, lowest j); groups are
// merged in ascending order with a strict compare, so the lowest word index wins every tie.
// |128 vr| < 2^30 for any u8 rows, so the key never overflows.
//
// Geometry.  A 256-thread workgroup owns 512 consecutive rows of the flattened [n_img * k_max]
// descriptor array: 4 waves x 4 query tiles of 32, the query descriptors converted in registers
// and held as the MFMA B operand (64 VGPRs) for the whole kernel.  The vocabulary, written once as
// i8 rows + key constants by the prep kernel and padded to a multiple of 128 with rows that can
// never win (zero row, crow = ROW_PAD), streams through LDS one 128-word group at a time: 16 KB of
// rows in the XOR-swizzled image K1 uses (conflict-free ds_read_b128) + 512 B of constants, double
// buffered through registers (the next group's global loads are issued before the MFMAs of the
// current one and stored to the other buffer after them).  MFMA output tile D[32 words][32
// queries]: the query is the lane, a lane's 16 accumulators are 16 of the 32 words, the other 16
// live in lane ^ 32; the two halves are merged once at the end (value, then lower index).
#include <climits>

#include "sfm_internal.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int D = 128;                 // bytes per descriptor / vocabulary row
constexpr int VA_WAVES = 4;            // waves per workgroup
constexpr int VA_QT = 4;               // query tiles (32 rows) per wave
constexpr int VA_QB = VA_WAVES * VA_QT * 32;   // 512 descriptor rows per workgroup
constexpr int VA_GROUP = 128;          // words per LDS stage = one row-key group
constexpr int VA_NK = D / 32;          // MFMA k-steps per tile
constexpr int VA_MAX_WORDS = 65536;
constexpr int VA_MAX_KMAX = 8192;
// crow of padded words: real keys are > -2^30, a padded word (zero row: dot = 0) has exactly this
constexpr int ROW_PAD = -(3 << 29);

__device__ __forceinline__ int swz(int row) { return (row >> 1) & 7; }

// Vocabulary prep: i8 rows (w ^ 0x80), padded with zero rows to nw_pad, and the row-key constant
// crow_j = -128 |w'_j|^2 + 127 - (j mod 128)  (ROW_PAD for the padding).
__global__ __launch_bounds__(256) void vocab_prep_kernel(const uint8_t* __restrict__ vocab,
                                                         int n_words, int nw_pad,
                                                         uint4* __restrict__ vocab_i8,
                                                         int32_t* __restrict__ crow) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nw_pad) return;
    uint4* o8 = vocab_i8 + (size_t)j * (D / 16);
    if (j >= n_words) {
#pragma unroll
        for (int q = 0; q < D / 16; ++q) o8[q] = make_uint4(0u, 0u, 0u, 0u);
        crow[j] = ROW_PAD;
        return;
    }
    const uint4* p = (const uint4*)(vocab + (size_t)j * D);
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
    crow[j] = -128 * nv + 127 - (j & 127);
}

__global__ __launch_bounds__(64 * VA_WAVES) void vocab_assign_kernel(
    const uint8_t* __restrict__ desc, const int32_t* __restrict__ n_kp, int k_max,
    long long n_rows, const uint4* __restrict__ vocab_i8, const int32_t* __restrict__ crow_tab,
    int n_group, int32_t* __restrict__ out_word, int32_t* __restrict__ out_dist) {
    // two stages of [128 words][128 B] + [128] key constants
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][VA_GROUP * D + VA_GROUP * 4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, r32 = lane & 31;
    const long long qbase = (long long)blockIdx.x * VA_QB + wave * (VA_QT * 32);

    // the wave's queries: B operand fragments (lane (r32, h) holds bytes [64 h, 64 h + 64) of row
    // r32 of each tile, 16 per k-step), |x'|^2 and validity
    v4i bq[VA_QT][VA_NK];
    int qn[VA_QT], B1[VA_QT], J1[VA_QT];
    bool valid[VA_QT];
#pragma unroll
    for (int c = 0; c < VA_QT; ++c) {
        const long long q = qbase + c * 32 + r32;
        valid[c] = false;
        if (q < n_rows) {
            const int img = (int)(q / k_max);
            valid[c] = (int)(q - (long long)img * k_max) < n_kp[img];
        }
        int nv = 0;
#pragma unroll
        for (int s = 0; s < VA_NK; ++s) {
            v4i x = {0, 0, 0, 0};
            if (valid[c]) {
                const v4i v = *(const v4i*)(desc + (size_t)q * D + 64 * h + 16 * s);
                x = v ^ (int)0x80808080u;
            }
            bq[c][s] = x;
            nv = __builtin_amdgcn_sdot4(x.x, x.x, nv, false);
            nv = __builtin_amdgcn_sdot4(x.y, x.y, nv, false);
            nv = __builtin_amdgcn_sdot4(x.z, x.z, nv, false);
            nv = __builtin_amdgcn_sdot4(x.w, x.w, nv, false);
        }
        qn[c] = nv + __shfl_xor(nv, 32);
        B1[c] = INT_MIN;
        J1[c] = -1;
    }

    // staging: 1024 16-B slots of rows + 32 of constants per group; thread t moves slots
    // t, t + 256, t + 512, t + 768 (row e / 8, slot e % 8, stored at the swizzled slot)
    uint4 pre0, pre1, pre2, pre3, prec = make_uint4(0u, 0u, 0u, 0u);
    const bool cthread = tid < VA_GROUP / 4;
#define VA_FETCH(g)                                                                   \
    do {                                                                              \
        const uint4* src_ = vocab_i8 + (size_t)(g) * (VA_GROUP * D / 16) + tid;       \
        pre0 = src_[0]; pre1 = src_[256]; pre2 = src_[512]; pre3 = src_[768];         \
        if (cthread) prec = ((const uint4*)(crow_tab + (size_t)(g) * VA_GROUP))[tid]; \
    } while (0)
    // slot e = tid + 256 i: row e >> 3 = (tid >> 3) + 32 i, so swz(row) does not depend on i
    const int st_off = (tid >> 3) * D + (((tid & 7) ^ swz(tid >> 3)) << 4);
#define VA_STORE(dst)                                                                 \
    do {                                                                              \
        *(uint4*)((dst) + st_off) = pre0;                                             \
        *(uint4*)((dst) + st_off + 32 * D) = pre1;                                    \
        *(uint4*)((dst) + st_off + 64 * D) = pre2;                                    \
        *(uint4*)((dst) + st_off + 96 * D) = pre3;                                    \
        if (cthread) *(uint4*)((dst) + VA_GROUP * D + tid * 16) = prec;               \
    } while (0)

    VA_FETCH(0);
    VA_STORE(lds[0]);
    __syncthreads();
    for (int g = 0; g < n_group; ++g) {
        const unsigned char* A = lds[g & 1];
        const int* Cr = (const int*)(A + VA_GROUP * D);
        if (g + 1 < n_group) VA_FETCH(g + 1);
        int tb[VA_QT];
#pragma unroll
        for (int c = 0; c < VA_QT; ++c) tb[c] = INT_MIN;
#pragma unroll 1
        for (int tt = 0; tt < VA_GROUP / 32; ++tt) {
            const int row = tt * 32 + r32;
            const int sw = swz(row);
            v4i af[VA_NK];
#pragma unroll
            for (int s = 0; s < VA_NK; ++s)
                af[s] = *(const v4i*)(A + row * D + (((4 * h + s) ^ sw) << 4));
            // accumulator r of lane (., h) is word row (r & 3) + 8 (r >> 2) + 4 h of the tile
            int crow[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const v4i cv = *(const v4i*)(Cr + tt * 32 + 8 * q + 4 * h);
                crow[4 * q + 0] = cv.x; crow[4 * q + 1] = cv.y;
                crow[4 * q + 2] = cv.z; crow[4 * q + 3] = cv.w;
            }
#pragma unroll
            for (int c = 0; c < VA_QT; c += 2) {
                v16i acc0 = {0}, acc1 = {0};
#pragma unroll
                for (int s = 0; s < VA_NK; ++s) {
                    acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[s], bq[c][s], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[s], bq[c + 1][s], acc1, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    tb[c] = max(tb[c], acc0[r] * 256 + crow[r]);
                    tb[c + 1] = max(tb[c + 1], acc1[r] * 256 + crow[r]);
                }
            }
        }
        // merge the group: strict compare in ascending group order keeps the lowest index
#pragma unroll
        for (int c = 0; c < VA_QT; ++c) {
            const int v1 = tb[c] >> 7;
            const int j1 = g * VA_GROUP + 127 - (tb[c] & 127);
            if (v1 > B1[c]) { B1[c] = v1; J1[c] = j1; }
        }
        if (g + 1 < n_group) VA_STORE(lds[(g + 1) & 1]);
        __syncthreads();
    }

#pragma unroll
    for (int c = 0; c < VA_QT; ++c) {
        const int P1 = __shfl_xor(B1[c], 32), PJ = __shfl_xor(J1[c], 32);
        if (P1 > B1[c] || (P1 == B1[c] && PJ < J1[c])) { B1[c] = P1; J1[c] = PJ; }
        const long long q = qbase + c * 32 + r32;
        if (h == 0 && q < n_rows) {
            out_word[q] = valid[c] ? J1[c] : -1;
            if (out_dist) out_dist[q] = valid[c] ? qn[c] - B1[c] : 0;   // d^2 = |x'|^2 - vr
        }
    }
}
#undef VA_FETCH
#undef VA_STORE

// Term frequencies: one block per (range of 16384 words, image); the image's words are counted
// into LDS with integer atomics and the whole range is written, so no memset and no dependence on
// the order of the atomics.
constexpr int BH_RANGE = 16384;
__global__ __launch_bounds__(256) void bow_hist_kernel(const int32_t* __restrict__ word,
                                                       const int32_t* __restrict__ n_kp, int k_max,
                                                       int n_words, uint16_t* __restrict__ out_hist) {
    __shared__ unsigned cnt[BH_RANGE];
    const int img = blockIdx.y, w0 = blockIdx.x * BH_RANGE, nw = min(BH_RANGE, n_words - w0);
    const int tid = threadIdx.x;
    for (int i = tid; i < nw; i += 256) cnt[i] = 0u;
    __syncthreads();
    const int n = min(max(n_kp[img], 0), k_max);
    const int32_t* wp = word + (size_t)img * k_max;
    for (int i = tid; i < n; i += 256) {
        const int w = wp[i] - w0;
        if (w >= 0 && w < nw) atomicAdd(&cnt[w], 1u);
    }
    __syncthreads();
    uint16_t* oh = out_hist + (size_t)img * n_words + w0;
    for (int i = tid; i < nw; i += 256) oh[i] = (uint16_t)cnt[i];
}

// Scores: one 256-thread block per 16 x 16 tile of image pairs, one pair per thread; the word axis
// streams through LDS in chunks of 512 (rows padded by one dword: at one word a wave reads 4 rows
// of ha, each broadcast to 16 lanes, and the 16 rows of hb, which sit in 16 different banks).
// score = sum_w min(tf_a, tf_b) * weight_w, exact in u64 (every term < 2^32).  The score is
// symmetric: only the tiles on and above the diagonal are computed (the others exit at once,
// block-uniformly and before any barrier) and every value is stored at (a, b) and (b, a); a
// diagonal tile writes each of its entries twice with the same value.
constexpr int BN_T = 16, BN_CH = 512, BN_LD = BN_CH + 2;
__global__ __launch_bounds__(256) void bow_score_kernel(const uint16_t* __restrict__ hist, int n_img,
                                                        int n_words,
                                                        const int32_t* __restrict__ weight,
                                                        long long* __restrict__ score) {
    __shared__ uint16_t ha[BN_T][BN_LD], hb[BN_T][BN_LD];
    __shared__ unsigned wt[BN_CH];
    if (blockIdx.x < blockIdx.y) return;   // below the diagonal: the mirrored tile stores it
    const int tid = threadIdx.x, ta = tid >> 4, tb = tid & 15;
    const int a0 = blockIdx.y * BN_T, b0 = blockIdx.x * BN_T;
    unsigned long long s = 0;
    for (int w0 = 0; w0 < n_words; w0 += BN_CH) {
        const int nw = min(BN_CH, n_words - w0);
        __syncthreads();
        for (int e = tid; e < BN_T * BN_CH; e += 256) {
            const int r = e / BN_CH, w = e % BN_CH;
            const bool in = w < nw;
            ha[r][w] = (in && a0 + r < n_img) ? hist[(size_t)(a0 + r) * n_words + w0 + w] : (uint16_t)0;
            hb[r][w] = (in && b0 + r < n_img) ? hist[(size_t)(b0 + r) * n_words + w0 + w] : (uint16_t)0;
        }
        for (int w = tid; w < BN_CH; w += 256) wt[w] = (w < nw) ? (unsigned)weight[w0 + w] : 0u;
        __syncthreads();
        for (int w = 0; w < nw; ++w) {
            const unsigned m = min((unsigned)ha[ta][w], (unsigned)hb[tb][w]);
            s += (unsigned long long)(m * wt[w]);
        }
    }
    const int a = a0 + ta, b = b0 + tb;
    if (a < n_img && b < n_img) {
        score[(size_t)a * n_img + b] = (long long)s;
        score[(size_t)b * n_img + a] = (long long)s;
    }
}

// Per image a: the up-to-k images b != a with the largest positive score, descending, lower b
// first among equals.  The rank of b is the number of candidates that precede it in that order,
// so every output slot is written by at most one thread.
__global__ __launch_bounds__(256) void bow_select_kernel(const long long* __restrict__ score,
                                                         int n_img, int k,
                                                         int32_t* __restrict__ out_nbr,
                                                         long long* __restrict__ out_score) {
    const int a = blockIdx.x, tid = threadIdx.x;
    const long long* row = score + (size_t)a * n_img;
    int32_t* on = out_nbr + (size_t)a * k;
    long long* os = out_score + (size_t)a * k;
    for (int i = tid; i < k; i += 256) { on[i] = -1; os[i] = 0; }
    __syncthreads();
    for (int b = tid; b < n_img; b += 256) {
        const long long sb = row[b];
        if (b == a || sb <= 0) continue;
        int rank = 0;
        for (int c = 0; c < n_img; ++c) {
            const long long sc = row[c];
            rank += (c != a) && (sc > sb || (sc == sb && c < b));
        }
        if (rank < k) { on[rank] = b; os[rank] = sb; }
    }
}

}  // namespace

extern "C" {

int sfm_vocab_assign(sfm_ctx* ctx, const uint8_t* desc, const int32_t* n_kp, int32_t n_img,
                     int32_t k_max, const uint8_t* vocab, int32_t n_words, int32_t* out_word,
                     int32_t* out_dist) {
    SFM_REQUIRE(ctx != nullptr, "sfm_vocab_assign: ctx is NULL");
    SFM_REQUIRE(n_img >= 0 && k_max >= 0, "sfm_vocab_assign: negative size");
    SFM_REQUIRE(n_words >= 1 && n_words <= VA_MAX_WORDS,
                "sfm_vocab_assign: n_words must be in [1, 65536]");
    SFM_REQUIRE(k_max <= VA_MAX_KMAX, "sfm_vocab_assign: k_max > 8192 not supported");
    const long long n_rows = (long long)n_img * k_max;
    if (n_rows == 0) return SFM_OK;
    SFM_REQUIRE(desc && n_kp && vocab && out_word, "sfm_vocab_assign: NULL array");
    SFM_REQUIRE((n_rows + VA_QB - 1) / VA_QB <= INT_MAX, "sfm_vocab_assign: too many descriptors");
    SFM_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int nw_pad = (int)sfm::align_up((size_t)n_words, VA_GROUP);
    const size_t vb = (size_t)nw_pad * D;
    char* ws = (char*)sfm::workspace(ctx, vb + (size_t)nw_pad * sizeof(int32_t));
    if (!ws) return SFM_ERR_NOMEM;
    uint4* vocab_i8 = (uint4*)ws;
    int32_t* crow = (int32_t*)(ws + vb);
    hipLaunchKernelGGL(vocab_prep_kernel, dim3((nw_pad + 255) / 256), dim3(256), 0, st, vocab,
                       n_words, nw_pad, vocab_i8, crow);
    SFM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(vocab_assign_kernel, dim3((unsigned)((n_rows + VA_QB - 1) / VA_QB)),
                       dim3(64 * VA_WAVES), 0, st, desc, n_kp, k_max, n_rows, vocab_i8, crow,
                       nw_pad / VA_GROUP, out_word, out_dist);
    SFM_HIP_CHECK(hipGetLastError());
    return SFM_OK;
}

int sfm_bow_hist(sfm_ctx* ctx, const int32_t* word, const int32_t* n_kp, int32_t n_img,
                 int32_t k_max, int32_t n_words, uint16_t* out_hist) {
    SFM_REQUIRE(ctx != nullptr, "sfm_bow_hist: ctx is NULL");
    SFM_REQUIRE(n_img >= 0 && k_max >= 0, "sfm_bow_hist: negative size");
    SFM_REQUIRE(n_words >= 1 && n_words <= VA_MAX_WORDS, "sfm_bow_hist: n_words must be in [1, 65536]");
    SFM_REQUIRE(k_max <= 65535, "sfm_bow_hist: k_max > 65535 does not fit a u16 term frequency");
    SFM_REQUIRE(n_img <= 65535, "sfm_bow_hist: n_img > 65535 not supported");
    if (n_img == 0) return SFM_OK;
    SFM_REQUIRE(n_kp && out_hist && (word || k_max == 0), "sfm_bow_hist: NULL array");
    SFM_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(bow_hist_kernel, dim3((n_words + BH_RANGE - 1) / BH_RANGE, n_img), dim3(256),
                       0, ctx->stream, word, n_kp, k_max, n_words, out_hist);
    SFM_HIP_CHECK(hipGetLastError());
    return SFM_OK;
}

int sfm_bow_neighbours(sfm_ctx* ctx, const uint16_t* hist, int32_t n_img, int32_t n_words,
                       const int32_t* weight, int32_t k, int32_t* out_nbr, int64_t* out_score) {
    SFM_REQUIRE(ctx != nullptr, "sfm_bow_neighbours: ctx is NULL");
    SFM_REQUIRE(n_img >= 0, "sfm_bow_neighbours: negative size");
    SFM_REQUIRE(n_words >= 1, "sfm_bow_neighbours: n_words must be >= 1");
    SFM_REQUIRE(k >= 1, "sfm_bow_neighbours: k must be >= 1");
    SFM_REQUIRE(n_img <= 16 * 65535, "sfm_bow_neighbours: n_img too large for the dense score matrix");
    if (n_img == 0) return SFM_OK;
    SFM_REQUIRE(hist && weight && out_nbr && out_score, "sfm_bow_neighbours: NULL array");
    SFM_HIP_CHECK(hipSetDevice(ctx->device));
    long long* score = (long long*)sfm::workspace(ctx, (size_t)n_img * n_img * sizeof(long long));
    if (!score) return SFM_ERR_NOMEM;
    const int nt = (n_img + BN_T - 1) / BN_T;
    hipLaunchKernelGGL(bow_score_kernel, dim3(nt, nt), dim3(256), 0, ctx->stream, hist, n_img,
                       n_words, weight, score);
    SFM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bow_select_kernel, dim3(n_img), dim3(256), 0, ctx->stream, score, n_img, k,
                       out_nbr, (long long*)out_score);
    SFM_HIP_CHECK(hipGetLastError());
    return SFM_OK;
}

}  // extern "C"
