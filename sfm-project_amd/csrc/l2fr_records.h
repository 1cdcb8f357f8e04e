// The ratio path's packed per-query records (match_l2fr.hip): 8 bytes each, host and device.
//
// Forward record (the scan's row top-2): e1, e2 as 23-bit two's-complement fields, "no real second
// element" as a cleared valid bit, the 32-train tile of e1 in 7 bits:
//     bits  0..22 e1 | 23..29 tile | 32..54 e2 | 55 e2 valid
// Result record (recovery / exact row scan): d1 in 23 bits, j1 in 12, the exact flag, the status:
//     bits  0..22 d1 | 32..43 j1 | 44 exact | 45..46 status
// A query the scan drops or leaves to the row scan has no result record until the compaction writes
// one for a row-scanned query: its class byte says which (CLS_DROP, CLS_SLOW; a candidate's class
// byte is its e1 tile).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define L2FR_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define L2FR_HD inline
#endif

namespace l2fr {

constexpr int REC_D = 128;       // features per descriptor
constexpr int REC_KMAX = 4096;   // rows per image
constexpr int E_BITS = 23, TILE_BITS = 7, J_BITS = 12, D1_BITS = 23;
// e = x'.y' - ceil(|y'|^2 / 2) over signed bytes: x'.y' in [-128*127*D, 128*128*D], |y'|^2 <= 128*128*D
constexpr long long E_HI = 128LL * 128 * REC_D;
constexpr long long E_LO = -128LL * 127 * REC_D - (128LL * 128 * REC_D + 1) / 2;
constexpr long long D1_HI = 255LL * 255 * REC_D;   // all 0 against all 255
static_assert(E_HI < (1LL << (E_BITS - 1)) && E_LO >= -(1LL << (E_BITS - 1)), "e needs more than E_BITS");
static_assert(REC_KMAX / 32 <= (1 << TILE_BITS), "tile needs more than TILE_BITS");
static_assert(REC_KMAX <= (1 << J_BITS), "j1 needs more than J_BITS");
static_assert(D1_HI < (1LL << D1_BITS), "d1 needs more than D1_BITS");

constexpr int E_NONE = -(1 << 23);   // unpacked e2 of "no real second element" (a real e is above)
static_assert(E_LO > E_NONE, "E_NONE must lie below every real e");

constexpr unsigned char CLS_SLOW = 0xFE, CLS_DROP = 0xFF;   // class bytes that are no tile
static_assert(REC_KMAX / 32 - 1 < CLS_SLOW, "a tile must not collide with a class sentinel");

constexpr uint32_t E_MASK = (1u << E_BITS) - 1u;

L2FR_HD int sext23(uint32_t v) {
    return (int32_t)(v << (32 - E_BITS)) >> (32 - E_BITS);   // arithmetic shift: sign-extends
}

struct Fwd { int e1, e2, tile; };   // e2 == E_NONE: no real second element

// e2 <= E_NONE (the scan's padding rows and untouched INT_MIN) packs as "none".
L2FR_HD uint64_t pack_fwd(int e1, int e2, int tile) {
    const uint32_t lo = ((uint32_t)e1 & E_MASK) | ((uint32_t)tile << E_BITS);
    const uint32_t hi = e2 > E_NONE ? (((uint32_t)e2 & E_MASK) | (1u << E_BITS)) : 0u;
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

L2FR_HD Fwd unpack_fwd(uint64_t v) {
    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    Fwd f;
    f.e1 = sext23(lo);
    f.tile = (int)((lo >> E_BITS) & ((1u << TILE_BITS) - 1u));
    f.e2 = ((hi >> E_BITS) & 1u) ? sext23(hi) : E_NONE;
    return f;
}

struct Res { int st, j1, d1, exact; };

L2FR_HD uint64_t pack_res(int st, int j1, int d1, int exact) {
    const uint32_t lo = (uint32_t)d1 & ((1u << D1_BITS) - 1u);
    const uint32_t hi = ((uint32_t)j1 & ((1u << J_BITS) - 1u)) | ((uint32_t)(exact & 1) << J_BITS) |
                        ((uint32_t)(st & 3) << (J_BITS + 1));
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

L2FR_HD Res unpack_res(uint64_t v) {
    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    Res r;
    r.d1 = (int)(lo & ((1u << D1_BITS) - 1u));
    r.j1 = (int)(hi & ((1u << J_BITS) - 1u));
    r.exact = (int)((hi >> J_BITS) & 1u);
    r.st = (int)((hi >> (J_BITS + 1)) & 3u);
    return r;
}

}  // namespace l2fr
