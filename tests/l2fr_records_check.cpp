// Host-only round trip of the ratio path's packed records (sfm-project_amd/csrc/l2fr_records.h):
// every field at its minimum, its maximum and its sentinel, and every combination of those.
// Built and run by test_l2fr_records_cpu.py with the host compiler under ASan + UBSan.
#include <climits>
#include <cstdio>
#include <vector>

#include "l2fr_records.h"

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);          \
            ++fails;                                                  \
        }                                                             \
    } while (0)

int main() {
    using namespace l2fr;
    // what the scan can produce: e in [E_LO, E_HI]; e2 also "none" as the padding rows leave it
    // (at or below E_NONE, down to the untouched INT_MIN)
    const std::vector<int> e1s = {(int)E_LO, (int)E_LO + 1, -1, 0, 1, (int)E_HI - 1, (int)E_HI,
                                  -(1 << 22) + 1, (1 << 21)};
    std::vector<int> e2s = e1s;
    const std::vector<int> none = {E_NONE, E_NONE - 1, -(1 << 30), -(1 << 30) + (int)E_HI, INT_MIN};
    const std::vector<int> tiles = {0, 1, 63, 64, REC_KMAX / 32 - 1};
    for (int e1 : e1s)
        for (int t : tiles) {
            for (int e2 : e2s) {
                const Fwd f = unpack_fwd(pack_fwd(e1, e2, t));
                CHECK(f.e1 == e1 && f.e2 == e2 && f.tile == t);
            }
            for (int e2 : none) {
                const Fwd f = unpack_fwd(pack_fwd(e1, e2, t));
                CHECK(f.e1 == e1 && f.e2 == E_NONE && f.tile == t);
                CHECK(!(f.e2 > E_NONE) && f.e2 != f.e1);
            }
        }
    // the smallest real e is above the sentinel, so "none" can never be taken for a value
    CHECK(E_LO > E_NONE);
    CHECK(unpack_fwd(pack_fwd(0, (int)E_LO, 0)).e2 == (int)E_LO);

    const std::vector<int> d1s = {0, 1, (int)D1_HI - 1, (int)D1_HI, (1 << D1_BITS) - 1};
    const std::vector<int> js = {0, 1, REC_KMAX / 2, REC_KMAX - 1};
    for (int st = 0; st < 4; ++st)
        for (int ex = 0; ex < 2; ++ex)
            for (int j : js)
                for (int d : d1s) {
                    const Res r = unpack_res(pack_res(st, j, d, ex));
                    CHECK(r.st == st && r.j1 == j && r.d1 == d && r.exact == ex);
                }
    // the fields do not overlap: each one alone leaves the others zero
    CHECK(unpack_res(pack_res(3, 0, 0, 0)).j1 == 0 && unpack_res(pack_res(3, 0, 0, 0)).exact == 0);
    CHECK(unpack_res(pack_res(0, REC_KMAX - 1, 0, 0)).st == 0);
    CHECK(unpack_res(pack_res(0, REC_KMAX - 1, 0, 0)).exact == 0);
    CHECK(unpack_res(pack_res(0, 0, (1 << D1_BITS) - 1, 0)).j1 == 0);
    CHECK(unpack_fwd(pack_fwd(-1, E_NONE, 0)).tile == 0);
    CHECK(unpack_fwd(pack_fwd(0, -1, 0)).e1 == 0 && unpack_fwd(pack_fwd(0, -1, 0)).tile == 0);
    CHECK(unpack_fwd(pack_fwd(0, E_NONE, REC_KMAX / 32 - 1)).e1 == 0);
    // class bytes: every tile is below the sentinels
    CHECK(REC_KMAX / 32 - 1 < CLS_SLOW && CLS_SLOW < CLS_DROP);
    if (fails) return 1;
    std::printf("l2fr records ok\n");
    return 0;
}
