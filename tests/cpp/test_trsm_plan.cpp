// The local Trsm paths (kernels.hpp trsm_plan, trsm_batched_ok): host-only,
// compiled against the HIP headers, no GPU.  These are the functions exec::Trsm,
// launch_trsm and TrsmLeft call, so a boundary that moves here moves the tests
// that name a path per shape (tests/_trsm_cases.py) with it.
#include "kernels.hpp"
#include <cstdio>

using elx::kern::i64;
using elx::kern::kTriInverseLdsMax;
using elx::kern::trsm_batched_ok;
using elx::kern::trsm_plan;
using elx::kern::TrsmPlan;

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

// the plan is usable in constant expressions (the kernels' launcher is host code too)
static_assert(trsm_plan(8, 129, 1).lds && !trsm_plan(8, 130, 1).lds, "f64 LDS boundary");
static_assert(trsm_plan(4, 259, 1).lds && !trsm_plan(4, 260, 1).lds, "f32 LDS boundary");

int main() {
    const size_t f64 = 8, f32 = 4;
    // the LDS kernel: m x 65 elements within 66 KiB
    EXPECT(trsm_plan(f64, 129, 7).lds && !trsm_plan(f64, 130, 7).lds, "f64 129/130");
    EXPECT(trsm_plan(f32, 259, 7).lds && !trsm_plan(f32, 260, 7).lds, "f32 259/260");
    EXPECT(trsm_plan(f64, 126, 9).lds_bytes <= 64 * 1024 && trsm_plan(f64, 127, 9).lds_bytes > 64 * 1024,
           "f64 crosses 64 KiB between 126 and 127 rows");
    EXPECT(trsm_plan(f32, 252, 9).lds_bytes <= 64 * 1024 && trsm_plan(f32, 253, 9).lds_bytes > 64 * 1024,
           "f32 crosses 64 KiB between 252 and 253 rows");
    // invert: n >= 4 m and m <= 256
    const i64 ms[] = {1, 2, 17, 64, 129, 130, 255, 256};
    for (i64 m : ms)
        for (size_t es : {f64, f32}) {
            EXPECT(!trsm_plan(es, m, 4 * m - 1).invert && trsm_plan(es, m, 4 * m).invert, "m %ld es %zu", (long)m, es);
            EXPECT(trsm_plan(es, m, 1 << 20).invert, "m %ld es %zu", (long)m, es);
        }
    for (size_t es : {f64, f32}) {
        EXPECT(trsm_plan(es, 256, 1024).invert && !trsm_plan(es, 257, 1028).invert, "es %zu 256/257", es);
        EXPECT(!trsm_plan(es, 257, 1 << 20).invert && !trsm_plan(es, 4096, 1 << 20).invert, "es %zu", es);
    }
    // lds depends on m alone, lds_bytes is exact, and an LDS launch stays within
    // what tri_inverse_batched_kernel (the same body) is allowed
    for (size_t es : {f64, f32})
        for (i64 m = 1; m <= 600; ++m) {
            const TrsmPlan a = trsm_plan(es, m, 1), b = trsm_plan(es, m, 4 * m);
            EXPECT(a.lds == b.lds && a.lds_bytes == b.lds_bytes, "m %ld es %zu", (long)m, es);
            EXPECT(a.lds_bytes == (size_t)m * 65 * es, "m %ld es %zu: %zu", (long)m, es, a.lds_bytes);
            EXPECT(!a.lds || a.lds_bytes <= (size_t)kTriInverseLdsMax, "m %ld es %zu", (long)m, es);
            EXPECT(a.lds == (a.lds_bytes <= 66 * 1024), "m %ld es %zu", (long)m, es);
            // the inverse on global memory: f64 m = 130..256 only; f32 never
            // (trsm_kernel<float, false, true> is unreachable through exec::Trsm)
            EXPECT((b.invert && !b.lds) == (es == f64 && m >= 130 && m <= 256), "m %ld es %zu", (long)m, es);
        }
    // the batched path: nb x 65 elements within kTriInverseLdsMax, width >= 4 nb, <= 65535 blocks
    struct { size_t es; i64 nb; bool fits; } const blocks[] = {
        {f64, 16, true},  {f32, 16, true},  {f64, 80, true},   {f32, 80, true},  {f64, 256, true},
        {f32, 256, true}, {f64, 295, true}, {f64, 296, false}, {f32, 590, true}, {f32, 591, false}};
    for (const auto& c : blocks) {
        const i64 m = 10 * c.nb + 3;
        EXPECT(trsm_batched_ok(c.es, c.nb, m, 4 * c.nb) == c.fits, "es %zu nb %ld", c.es, (long)c.nb);
        EXPECT(trsm_batched_ok(c.es, c.nb, m, 100 * c.nb) == c.fits, "es %zu nb %ld", c.es, (long)c.nb);
        EXPECT(!trsm_batched_ok(c.es, c.nb, m, 4 * c.nb - 1), "es %zu nb %ld: width 4nb-1", c.es, (long)c.nb);
        EXPECT(!trsm_batched_ok(c.es, c.nb, m, 0), "es %zu nb %ld: width 0", c.es, (long)c.nb);
    }
    // gridDim.y: at most 65535 diagonal blocks
    EXPECT(trsm_batched_ok(f64, 16, (i64)65535 * 16, 64), "65535 blocks");
    EXPECT(!trsm_batched_ok(f64, 16, (i64)65535 * 16 + 1, 64), "65536 blocks");
    EXPECT(trsm_batched_ok(f64, 1, 65535, 4) && !trsm_batched_ok(f64, 1, 65536, 4), "nb 1");
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
