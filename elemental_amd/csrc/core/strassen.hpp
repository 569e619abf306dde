// One or two Strassen-Winograd levels over the local GEMM:
// C := alpha op(A) op(B) + beta C as seven half-size products and 15 quadrant
// additions, for the large f64 / f32 products whose plain kernel already runs
// at the MFMA limit.  The schedule is written over exec:: operations (GemmPlain,
// QuadSum, QuadScatter), so it runs on either device; DESIGN.md section 3.
#pragma once
#include "../common.hpp"
#include "../runtime/runtime.hpp"

namespace elx {
namespace strassen {

// The default threshold on min(m, n, k).  The measured crossover against the
// plain kernels lies between 6144^3 (one level 6 % slower) and 8192^3 (5 % faster
// in every orientation, f64 and f32), and the default is
// never below kMinFloor, so the blocks of LU, QR, Trsm, Cholesky and Trrk keep
// the code they ran before: the floor it is.
constexpr Int kMinFloor = 8192;
constexpr Int kDefaultMin = kMinFloor;
// The inner threshold: a sub-product of the first level splits again only when
// its own min(m, n, k) reaches it.  The same crossover, so by default the second
// level runs where the outer min(m, n, k) >= 16384 (32768^3: 814.0 -> 743.7 ms,
// 16384^3: 104.4 -> 99.5 ms in f64, 52.2 -> 49.7 ms in f32) and never splits the
// 4096^3 and 6144^3 sub-products that lose (profiles/strassen_crossover_ab.txt).
constexpr Int kDefaultMin2 = kMinFloor;

// Read from the environment at every call:
//   ELX_GEMM_STRASSEN       levels: 0 off, 1, 2.  Unset: up to two, the second
//                           under the inner threshold's own default
//   ELX_GEMM_STRASSEN_MIN   the outer threshold on min(m, n, k) (tests, A/B runs);
//                           on Device::CPU the path runs only when this is set.
//                           With ELX_GEMM_STRASSEN=2 it is the inner one as well
//   ELX_GEMM_STRASSEN_MIN2  the inner threshold, on a sub-product's min(m, n, k)
struct Knobs {
    int levels;
    Int min;
    Int min2;
    bool forced;  // ELX_GEMM_STRASSEN_MIN is set
};
Knobs ReadKnobs();

// The one eligibility test (the workspace apart): f64 / f32, even m, n, k,
// min(m, n, k) >= the threshold, alpha != 0, the GPU device or a forced threshold
bool Eligible(Device dev, DType t, Int m, Int n, Int k, double alpha, const Knobs& kn);

// Runs the product with up to `levels` levels and returns how many were used;
// 0: not eligible or no workspace, and nothing was written (the caller runs the
// plain kernel).  The order of operations is fixed: equal calls give equal bits.
int Gemm(int levels, const Knobs& kn, Device dev, DType t, bool ta, bool tb, Int m, Int n, Int k, double alpha,
         const void* A, Int lda, const void* B, Int ldb, double beta, void* C, Int ldc, hipStream_t s);

}  // namespace strassen
}  // namespace elx
