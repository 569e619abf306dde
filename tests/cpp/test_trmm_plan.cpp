// The k range trmm_tri's row tiles walk (kernels.hpp trmm_krange): host-only,
// compiled against the HIP headers, no GPU.
#include "kernels.hpp"
#include <cstdio>

using elx::kern::i64;
using elx::kern::trmm_krange;
using elx::kern::TrmmKRange;

static int fails = 0;
#define EXPECT(c, ...)                          \
    do {                                        \
        if (!(c)) {                             \
            ++fails;                            \
            std::printf("FAIL %s: ", #c);       \
            std::printf(__VA_ARGS__);           \
            std::printf("\n");                  \
        }                                       \
    } while (0)

int main() {
    const i64 bk = elx::kern::kTrmmBK;
    const i64 bms[] = {elx::kern::kTrmmBM64, elx::kern::kTrmmBM32};
    const i64 ms[] = {1, 16, 17, 128, 129, 300};
    for (i64 bm : bms) {
        EXPECT(bm % bk == 0, "bm %ld", (long)bm);
        for (int op_lower = 0; op_lower < 2; ++op_lower) {
            for (i64 m : ms) {
                for (i64 i0 = 0; i0 < m; i0 += bm) {
                    const TrmmKRange r = trmm_krange(op_lower != 0, m, i0, bm);
                    const i64 i1 = i0 + bm < m ? i0 + bm : m;  // the tile's rows [i0, i1)
                    EXPECT(r.k0 % bk == 0 && 0 <= r.k0 && r.k0 < r.k1 && r.k1 <= m, "m %ld i0 %ld: [%ld, %ld)", (long)m,
                           (long)i0, (long)r.k0, (long)r.k1);
                    // every k with a stored element op(A)(i,k), i in the tile's rows, is inside
                    for (i64 i = i0; i < i1; ++i)
                        for (i64 k = 0; k < m; ++k)
                            if (op_lower ? k <= i : k >= i)
                                EXPECT(r.k0 <= k && k < r.k1, "m %ld bm %ld lower %d: (%ld,%ld) outside [%ld,%ld)",
                                       (long)m, (long)bm, op_lower, (long)i, (long)k, (long)r.k0, (long)r.k1);
                    // and the range ends within a slab plus a tile height of the triangle:
                    // stored k of these rows span [0, i1) (lower) or [i0, m) (upper)
                    if (op_lower) EXPECT(r.k0 == 0 && r.k1 <= i1 - 1 + bk + bm, "m %ld i0 %ld", (long)m, (long)i0);
                    else EXPECT(r.k1 == m && r.k0 >= i0 - bk - bm, "m %ld i0 %ld", (long)m, (long)i0);
                }
            }
            // slabs walked at m = 4096 against the full product's (a condition on the
            // plan: the exact triangle gives 0.5 + bm/(2m) + bk/(2m))
            const i64 m = 4096;
            i64 tri = 0, full = 0;
            for (i64 i0 = 0; i0 < m; i0 += bm) {
                const TrmmKRange r = trmm_krange(op_lower != 0, m, i0, bm);
                tri += (r.k1 - r.k0 + bk - 1) / bk;
                full += (m + bk - 1) / bk;
            }
            EXPECT(10 * tri <= 6 * full, "bm %ld lower %d: %ld of %ld slabs", (long)bm, op_lower, (long)tri, (long)full);
        }
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
