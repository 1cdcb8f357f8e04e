// Image retrieval for binary descriptors (DESIGN.md §4.11 "Hamming"): the nearest vocabulary word
// of every 256-bit descriptor under Hamming distance, and one k-majority round of vocabulary
// refinement.  Integer and exact: every output is a function of the inputs alone.
//
// sfm_vocab_assign_hamming — vocab_assign_kernel's geometry (retrieval.hip) at twice the depth.
// Every bit becomes one byte of value 0 or 16, so a 256-bit row is 256 i8 and a product of two set
// bits is 256:  with n_q, n_w the bit counts and c the common set bits, d = n_q + n_w - 2 c, and the
// nearest word maximises vr = 2 c - n_w.  The accumulator of v_mfma_i32_32x32x32_i8 starts from the
// word's key constant (ham_key_kernel's form, match_hamming.hip), so after the 8 k-steps it holds
//     Kr = 256 c + crow_j,   crow_j = -128 n_w + 127 - (j mod 128)   =   128 vr + (127 - j mod 128)
// with no VALU op: a plain max over a group of 128 words yields (largest vr, lowest j); groups are
// merged in ascending order with a strict compare, the two lane halves by (vr, then lower index),
// so the lowest word index wins every tie.  |Kr| <= 2^16, padded words carry ROW_PAD and a zero
// row, so they lose against every real word.
//
// Geometry.  A 256-thread workgroup owns 256 consecutive rows of the flattened descriptor array:
// 4 waves x 2 query tiles of 32, expanded in registers and held as the MFMA B operand (64 VGPRs).
// The vocabulary is read PACKED from global memory, 4 KB per 128-word group and one 16-B load per
// thread, and expanded on the way into LDS: 32 KB of rows (16-B slot s of row r stored at slot
// s ^ (r & 15): 256-B rows all start on bank 0, and the 16 lanes of a ds_read_b128 group hold 16
// different r & 15) + 512 B of key constants, which the staging threads compute from the bit
// counts they have in hand.  Double buffered through registers: the next group's load is issued
// before the MFMAs of the current one, expanded and stored after them.
//
// Bit order: expanded dword (d, k) of a row is ((x_d >> k) & 0x01010101) << 4 for packed dword
// x_d, d = 0..7, k = 0..7, at 16-B slot 2 d + (k >> 2), dword k & 3.  Queries and words use the
// same order, and a Hamming distance does not depend on it.
#include <climits>

#include "sfm_internal.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int DP = 32;                  // packed bytes per row
constexpr int DX = 256;                 // expanded bytes per row
constexpr int VH_WAVES = 4;
constexpr int VH_QT = 2;                // query tiles (32 rows) per wave
constexpr int VH_QB = VH_WAVES * VH_QT * 32;   // 256 descriptor rows per workgroup
constexpr int VH_GROUP = 128;           // words per LDS stage = one row-key group
constexpr int VH_NK = DX / 32;          // 8 MFMA k-steps per tile
constexpr int VH_MAX_WORDS = 65536;
constexpr int VH_MAX_KMAX = 8192;
constexpr int ROW_PAD = -(3 << 29);     // real keys are >= -2^15

// bit k of every byte of x, as 0 / 16 in that byte
template <int K>
__device__ __forceinline__ int spread(unsigned x) {
    if constexpr (K <= 4) return (int)((x << (4 - K)) & 0x10101010u);
    else return (int)((x >> (K - 4)) & 0x10101010u);
}

// the four 16-B slots that two packed dwords expand to; slot 2 e + u holds bits 4 u .. 4 u + 3
__device__ __forceinline__ v4i slot_lo(unsigned x) {
    return v4i{spread<0>(x), spread<1>(x), spread<2>(x), spread<3>(x)};
}
__device__ __forceinline__ v4i slot_hi(unsigned x) {
    return v4i{spread<4>(x), spread<5>(x), spread<6>(x), spread<7>(x)};
}

__device__ __forceinline__ int popc4(const uint4& v) {
    return __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
}

__global__ __launch_bounds__(64 * VH_WAVES) void vocab_assign_hamming_kernel(
    const uint8_t* __restrict__ desc, const int32_t* __restrict__ n_kp, int k_max,
    long long n_rows, const uint8_t* __restrict__ vocab, int n_words, int n_group,
    int32_t* __restrict__ out_word, int32_t* __restrict__ out_dist) {
    // two stages of [128 words][256 B] + [128] key constants
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][VH_GROUP * DX + VH_GROUP * 4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, r32 = lane & 31;
    const long long qbase = (long long)blockIdx.x * VH_QB + wave * (VH_QT * 32);

    // the wave's queries: lane (r32, h) holds packed dwords [4 h, 4 h + 4) of row r32 of each tile,
    // expanded to slots 8 h + s, one per k-step s
    v4i bq[VH_QT][VH_NK];
    int qn[VH_QT], B1[VH_QT], J1[VH_QT];
    bool valid[VH_QT];
#pragma unroll
    for (int c = 0; c < VH_QT; ++c) {
        const long long q = qbase + c * 32 + r32;
        valid[c] = false;
        if (q < n_rows) {
            const int img = (int)(q / k_max);
            valid[c] = (int)(q - (long long)img * k_max) < n_kp[img];
        }
        uint4 x = make_uint4(0u, 0u, 0u, 0u);
        if (valid[c]) x = *(const uint4*)(desc + (size_t)q * DP + 16 * h);
        bq[c][0] = slot_lo(x.x); bq[c][1] = slot_hi(x.x);
        bq[c][2] = slot_lo(x.y); bq[c][3] = slot_hi(x.y);
        bq[c][4] = slot_lo(x.z); bq[c][5] = slot_hi(x.z);
        bq[c][6] = slot_lo(x.w); bq[c][7] = slot_hi(x.w);
        const int nv = popc4(x);
        qn[c] = nv + __shfl_xor(nv, 32);
        B1[c] = INT_MIN;
        J1[c] = -1;
    }

    // staging: thread t moves half p = t & 1 (packed dwords [4 p, 4 p + 4), slots 8 p + s) of word
    // t >> 1 of the group; the even thread of a word also writes its key constant
    const int wl = tid >> 1, p = tid & 1;
    uint4 pre;
    int prec;
#define VH_FETCH(g)                                                                   \
    do {                                                                              \
        const int j_ = (g) * VH_GROUP + wl;                                           \
        pre = make_uint4(0u, 0u, 0u, 0u);                                             \
        if (j_ < n_words) pre = *(const uint4*)(vocab + (size_t)j_ * DP + 16 * p);    \
        const int nh_ = popc4(pre);                                                   \
        const int nw_ = nh_ + __shfl_xor(nh_, 1);                                     \
        prec = j_ < n_words ? -128 * nw_ + 127 - wl : ROW_PAD;                        \
    } while (0)
    const int st_row = wl * DX, st_sw = wl & 15;
#define VH_SLOT(dst, s, v) *(v4i*)((dst) + st_row + (((8 * p + (s)) ^ st_sw) << 4)) = (v)
#define VH_STORE(dst)                                                                 \
    do {                                                                              \
        VH_SLOT(dst, 0, slot_lo(pre.x)); VH_SLOT(dst, 1, slot_hi(pre.x));             \
        VH_SLOT(dst, 2, slot_lo(pre.y)); VH_SLOT(dst, 3, slot_hi(pre.y));             \
        VH_SLOT(dst, 4, slot_lo(pre.z)); VH_SLOT(dst, 5, slot_hi(pre.z));             \
        VH_SLOT(dst, 6, slot_lo(pre.w)); VH_SLOT(dst, 7, slot_hi(pre.w));             \
        if (p == 0) *(int*)((dst) + VH_GROUP * DX + wl * 4) = prec;                   \
    } while (0)

    VH_FETCH(0);
    VH_STORE(lds[0]);
    __syncthreads();
    for (int g = 0; g < n_group; ++g) {
        const unsigned char* A = lds[g & 1];
        const int* Cr = (const int*)(A + VH_GROUP * DX);
        if (g + 1 < n_group) VH_FETCH(g + 1);
        int tb[VH_QT];
#pragma unroll
        for (int c = 0; c < VH_QT; ++c) tb[c] = INT_MIN;
#pragma unroll 1
        for (int tt = 0; tt < VH_GROUP / 32; ++tt) {
            const int row = tt * 32 + r32;
            const int sw = row & 15;
            v4i af[VH_NK];
#pragma unroll
            for (int s = 0; s < VH_NK; ++s)
                af[s] = *(const v4i*)(A + row * DX + (((8 * h + s) ^ sw) << 4));
            // accumulator r of lane (., h) is word row (r & 3) + 8 (r >> 2) + 4 h of the tile
            v16i crow;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const v4i cv = *(const v4i*)(Cr + tt * 32 + 8 * q + 4 * h);
                crow[4 * q + 0] = cv.x; crow[4 * q + 1] = cv.y;
                crow[4 * q + 2] = cv.z; crow[4 * q + 3] = cv.w;
            }
            v16i acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[0], bq[0][0], crow, 0, 0, 0);
            v16i acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[0], bq[1][0], crow, 0, 0, 0);
#pragma unroll
            for (int s = 1; s < VH_NK; ++s) {
                acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[s], bq[0][s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[s], bq[1][s], acc1, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                tb[0] = max(tb[0], acc0[r]);
                tb[1] = max(tb[1], acc1[r]);
            }
        }
        // merge the group: strict compare in ascending group order keeps the lowest index
#pragma unroll
        for (int c = 0; c < VH_QT; ++c) {
            const int v1 = tb[c] >> 7;
            const int j1 = g * VH_GROUP + 127 - (tb[c] & 127);
            if (v1 > B1[c]) { B1[c] = v1; J1[c] = j1; }
        }
        if (g + 1 < n_group) VH_STORE(lds[(g + 1) & 1]);
        __syncthreads();
    }

#pragma unroll
    for (int c = 0; c < VH_QT; ++c) {
        const int P1 = __shfl_xor(B1[c], 32), PJ = __shfl_xor(J1[c], 32);
        if (P1 > B1[c] || (P1 == B1[c] && PJ < J1[c])) { B1[c] = P1; J1[c] = PJ; }
        const long long q = qbase + c * 32 + r32;
        if (h == 0 && q < n_rows) {
            out_word[q] = valid[c] ? J1[c] : -1;
            if (out_dist) out_dist[q] = valid[c] ? qn[c] - B1[c] : 0;   // d = n_q - vr
        }
    }
}
#undef VH_FETCH
#undef VH_SLOT
#undef VH_STORE

// k-majority, pass 1: per word the member count and per bit the number of members that have it
// set, by integer atomics into zeroed counters (sums do not depend on their order).  A block takes
// 32 consecutive rows, thread b bit b (byte b >> 3, bit b & 7); everything but the bit test is
// block-uniform.
constexpr int MJ_ROWS = 32;
__global__ __launch_bounds__(256) void majority_count_kernel(
    const uint8_t* __restrict__ desc, const int32_t* __restrict__ n_kp, int k_max, long long n_rows,
    const int32_t* __restrict__ word, int n_words, unsigned* __restrict__ ones,
    unsigned* __restrict__ cnt) {
    const int b = threadIdx.x;
    const long long q0 = (long long)blockIdx.x * MJ_ROWS;
    for (int i = 0; i < MJ_ROWS; ++i) {
        const long long q = q0 + i;
        if (q >= n_rows) break;
        const int img = (int)(q / k_max);
        if ((int)(q - (long long)img * k_max) >= n_kp[img]) continue;
        const int w = word[q];
        if (w < 0 || w >= n_words) continue;
        if ((desc[(size_t)q * DP + (b >> 3)] >> (b & 7)) & 1) atomicAdd(&ones[(size_t)w * 256 + b], 1u);
        if (b == 0) atomicAdd(&cnt[w], 1u);
    }
}

// pass 2: one thread per (word, byte).  Bit = 1 if 2 ones > cnt, the old bit if 2 ones == cnt
// (which also keeps a word without members as it is), else 0.
__global__ __launch_bounds__(256) void majority_write_kernel(
    const uint8_t* __restrict__ vocab, int n_words, const unsigned* __restrict__ ones,
    const unsigned* __restrict__ cnt, uint8_t* __restrict__ out_vocab) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_words * DP) return;
    const unsigned long long c = cnt[e >> 5];
    const unsigned old = vocab[e];
    const unsigned* o = ones + (size_t)e * 8;
    unsigned out = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned long long t = 2ull * o[i];
        out |= (t > c ? 1u : (t == c ? (old >> i) & 1u : 0u)) << i;
    }
    out_vocab[e] = (uint8_t)out;
}

}  // namespace

extern "C" {

int sfm_vocab_assign_hamming(sfm_ctx* ctx, const uint8_t* desc, const int32_t* n_kp, int32_t n_img,
                             int32_t k_max, const uint8_t* vocab, int32_t n_words,
                             int32_t* out_word, int32_t* out_dist) {
    SFM_REQUIRE(ctx != nullptr, "sfm_vocab_assign_hamming: ctx is NULL");
    SFM_REQUIRE(n_img >= 0 && k_max >= 0, "sfm_vocab_assign_hamming: negative size");
    SFM_REQUIRE(n_words >= 1 && n_words <= VH_MAX_WORDS,
                "sfm_vocab_assign_hamming: n_words must be in [1, 65536]");
    SFM_REQUIRE(k_max <= VH_MAX_KMAX, "sfm_vocab_assign_hamming: k_max > 8192 not supported");
    const long long n_rows = (long long)n_img * k_max;
    if (n_rows == 0) return SFM_OK;
    SFM_REQUIRE(desc && n_kp && vocab && out_word, "sfm_vocab_assign_hamming: NULL array");
    SFM_REQUIRE(((uintptr_t)desc | (uintptr_t)vocab) % 16 == 0,
                "sfm_vocab_assign_hamming: desc and vocab must be 16-byte aligned");
    SFM_REQUIRE((n_rows + VH_QB - 1) / VH_QB <= INT_MAX,
                "sfm_vocab_assign_hamming: too many descriptors");
    SFM_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(vocab_assign_hamming_kernel, dim3((unsigned)((n_rows + VH_QB - 1) / VH_QB)),
                       dim3(64 * VH_WAVES), 0, ctx->stream, desc, n_kp, k_max, n_rows, vocab,
                       n_words, (n_words + VH_GROUP - 1) / VH_GROUP, out_word, out_dist);
    SFM_HIP_CHECK(hipGetLastError());
    return SFM_OK;
}

int sfm_vocab_majority(sfm_ctx* ctx, const uint8_t* desc, const int32_t* n_kp, int32_t n_img,
                       int32_t k_max, const int32_t* word, const uint8_t* vocab, int32_t n_words,
                       uint8_t* out_vocab) {
    SFM_REQUIRE(ctx != nullptr, "sfm_vocab_majority: ctx is NULL");
    SFM_REQUIRE(n_img >= 0 && k_max >= 0, "sfm_vocab_majority: negative size");
    SFM_REQUIRE(n_words >= 1 && n_words <= VH_MAX_WORDS,
                "sfm_vocab_majority: n_words must be in [1, 65536]");
    SFM_REQUIRE(vocab && out_vocab, "sfm_vocab_majority: NULL array");
    const long long n_rows = (long long)n_img * k_max;
    SFM_REQUIRE(n_rows == 0 || (desc && n_kp && word), "sfm_vocab_majority: NULL array");
    SFM_REQUIRE(n_rows < (1ll << 32), "sfm_vocab_majority: too many descriptors for u32 counters");
    SFM_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t cb = ((size_t)n_words * 256 + n_words) * sizeof(unsigned);
    unsigned* ones = (unsigned*)sfm::workspace(ctx, cb);
    if (!ones) return SFM_ERR_NOMEM;
    unsigned* cnt = ones + (size_t)n_words * 256;
    SFM_HIP_CHECK(hipMemsetAsync(ones, 0, cb, st));
    if (n_rows > 0) {
        hipLaunchKernelGGL(majority_count_kernel, dim3((unsigned)((n_rows + MJ_ROWS - 1) / MJ_ROWS)),
                           dim3(256), 0, st, desc, n_kp, k_max, n_rows, word, n_words, ones, cnt);
        SFM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(majority_write_kernel, dim3((n_words * DP + 255) / 256), dim3(256), 0, st,
                       vocab, n_words, ones, cnt, out_vocab);
    SFM_HIP_CHECK(hipGetLastError());
    return SFM_OK;
}

}  // extern "C"
