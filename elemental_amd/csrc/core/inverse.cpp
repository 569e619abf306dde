// El::TriangularInverse, El::Trtrmm and El::HPDInverse on DistMatrices.
#include "level3_internal.hpp"
#include "exec.hpp"
#include <algorithm>
#include <cstdlib>
#include <functional>
#include "../runtime/trace.hpp"

namespace elx {

using namespace detail;

namespace {

void RequireSquareReal(const DistMatrix& A, const char* who) {
    if (A.Height() != A.Width()) throw LogicError("A must be square");
    RequireReal(A.Type(), who);
}

Int LeafRows() { return std::max<Int>(1, std::min<Int>(Blocksize(), kern::kTrtriMax)); }

// The split both drivers share with Cholesky's `factor`: [K0, K1) is cut at a
// multiple of nb from K0 until one block of at most nb rows is left.  pre runs
// before the two halves of a cut and mid between them; kernel on a single block,
// staged as A11[*,*] where the local storage is not already that layout.
//
// Where A's local block is the whole matrix (a 1x1 grid) the recursion stops at
// blocks of ELX_INVERSE_SWEEP rows (default 4096; 0: recurse down to single
// leaves; read per call, for A/B) and `sweep` takes such a block leaf by leaf
// with direct launches on the local buffer: the same panel operations, but
// each leaf's two Trsm calls (or its Trmm) become GEMMs with the block the leaf
// kernel has just inverted (or multiplied).  Measured at n = 16384 f64 on a 1x1
// GPU grid (profiles/hpd_inverse_bench.log): HPDInverse 242.2 ms without, 153.9
// ms with.  Host time is not what it saves (5 % of the wall time without):
// Trsm on a 128-row view runs the per-lane substitution kernels, 110 ms of the
// 235 ms of kernel time without the sweeps.  Blocks of 4096 rows measured best
// (512: 179.2 ms, 1024: 165.5, 2048: 160.9, 4096: 154.2, 8192: 155.0, all: 177.9).
struct Split {
    DistMatrix& A;
    Int nb;
    std::function<void(DistMatrix&, Int)> kernel;       // on the staged block and its order
    std::function<void(Int, Int, Int)> pre, mid;        // (K0, cut, K1); either may be empty
    std::function<void(Int, Int)> sweep;                // (K0, K1)
    std::shared_ptr<DistMatrix> stage = A.Like(Dist::STAR, Dist::STAR);
    Int sweep_rows = SweepRows(A);

    static Int SweepRows(const DistMatrix& A) {
        const Int n = A.Height();
        const bool local = SameLocalLayout(A, Dist::STAR, Dist::STAR, 0, 0) && A.LocalHeight() == n &&
                           A.LocalWidth() == n && A.LDim() > 0;
        const char* s = getenv("ELX_INVERSE_SWEEP");
        return local ? (s ? (Int)atoll(s) : (Int)4096) : 0;
    }

    void leaf(Int k0, Int k1) {
        auto A11 = DistMatrix::View(A, k0, k1, k0, k1);
        DistMatrix& a11 = StageDiagonalBlock(*A11, *stage);
        kernel(a11, k1 - k0);
        if (&a11 != A11.get()) Copy(a11, *A11);  // A11[MC,MR] <- A11[*,*]
    }
    void run(Int K0, Int K1) {
        const Int nbk = (K1 - K0 + nb - 1) / nb;
        if (nbk <= 1) return leaf(K0, K1);
        if (K1 - K0 <= sweep_rows) return sweep(K0, K1);
        const Int cut = K0 + (nbk / 2) * nb;
        if (pre) pre(K0, cut, K1);
        run(K0, cut);
        if (mid) mid(K0, cut, K1);
        run(cut, K1);
    }
};

// The local buffer of a matrix whose local block is the whole matrix, and the
// workspaces of a sweep over it.
struct LocalPanels {
    DistMatrix& A;
    Int ycap;  // elements of y to start with: the largest panel of a sweep
    const Device dev = A.Dev();
    const DType t = A.Type();
    const size_t es = DTypeSize(t);
    const Int ld = A.LDim();
    hipStream_t s = A.Stream();
    Buffer w, y, ttmp;

    char* at(Int i, Int j) const { return static_cast<char*>(A.Buffer()) + (i + j * ld) * es; }
    // W (kb x kb, leading dimension kb) := the uplo triangle of the block at
    // (k0, k0), zeros in the other triangle and ones on a unit diagonal
    void* FullTriangle(bool lower, bool unit, Int k0, Int kb) {
        if (w.bytes() < static_cast<size_t>(kb * kb) * es) w.Reset(dev, kb * kb * es, s);
        exec::Fill(dev, t, kb, kb, 0.0, w.data(), kb, s);
        exec::Trapezoid(dev, t, lower, kb, kb, 1.0, at(k0, k0), ld, 0.0, w.data(), kb, 0, 1, 0, 1,
                        unit ? (lower ? -1 : 1) : 0, s);
        if (unit) exec::Fill(dev, t, 1, kb, 1.0, w.data(), kb + 1, s);
        return w.data();
    }
    // P (m x n at (i, j)) := alpha op(X) op(Z) through the workspace: one GEMM and one copy
    void Assign(Int i, Int j, Int m, Int n, Int k, double alpha, bool tx, const void* X, Int ldx, bool tz,
                const void* Z, Int ldz) {
        if (m <= 0 || n <= 0) return;
        if (y.bytes() < static_cast<size_t>(m * n) * es) y.Reset(dev, std::max(m * n, ycap) * es, s);
        exec::Gemm(dev, t, tx, tz, m, n, k, alpha, X, ldx, Z, ldz, 0.0, y.data(), m, s);
        const kern::Copy2D back{m, n, y.data(), 1, m, at(i, j), 1, ld};
        exec::Copy2DBatch(dev, t, &back, 1, false, 0.0, s);
    }
};

// On A in [MC,MR].  With halves 1 and 2 of a cut, X21 = -L22^-1 L21 L11^-1
// (X12 = -U11^-1 U12 U22^-1): the two Trsm calls are the reference's per-panel
// operations (LVar3.hpp:69-72, UVar3.hpp) regrouped so that half of the FLOPs
// are two n/2 solves, and they read the diagonal blocks un-inverted, so they
// come before the recursion into those.
void TriangularInverseMCMR(bool lower, int diag, DistMatrix& A) {
    const bool unit = diag == ELX_UNIT;
    Split sp{A, LeafRows()};
    sp.kernel = [&](DistMatrix& a11, Int kb) {
        exec::TriangularInverse(A.Dev(), A.Type(), lower, unit, kb, a11.Buffer(), std::max<Int>(1, a11.LDim()),
                                a11.Stream());
    };
    sp.pre = [&](Int k0, Int cut, Int k1) {
        auto A11 = DistMatrix::View(A, k0, cut, k0, cut);
        auto A22 = DistMatrix::View(A, cut, k1, cut, k1);
        if (lower) {
            auto A21 = DistMatrix::View(A, cut, k1, k0, cut);
            Trsm(ELX_LEFT, ELX_LOWER, ELX_NORMAL, diag, -1.0, *A22, *A21);
            Trsm(ELX_RIGHT, ELX_LOWER, ELX_NORMAL, diag, 1.0, *A11, *A21);
        } else {
            auto A12 = DistMatrix::View(A, k0, cut, cut, k1);
            Trsm(ELX_LEFT, ELX_UPPER, ELX_NORMAL, diag, -1.0, *A11, *A12);
            Trsm(ELX_RIGHT, ELX_UPPER, ELX_NORMAL, diag, 1.0, *A22, *A12);
        }
    };
    // triang_inv::LVar3 / UVar3 (LVar3.hpp:56-73) on A(K0:K1, K0:K1), one leaf per
    // step, with W = the inverted diagonal block in place of the two Trsm calls:
    //   lower: L10 := -W L10;  L20 += L21 L10;  L21 := L21 W
    //   upper: U01 := -U01 W;  U02 += U01 U12;  U12 := W U12
    LocalPanels lp{A, sp.sweep_rows * sp.nb};
    sp.sweep = [&](Int K0, Int K1) {
        for (Int k0 = K0; k0 < K1; k0 += sp.nb) {
            const Int k1 = std::min(K1, k0 + sp.nb), kb = k1 - k0, p = k0 - K0, rest = K1 - k1;
            exec::TriangularInverse(lp.dev, lp.t, lower, unit, kb, lp.at(k0, k0), lp.ld, lp.s);
            if (p == 0 && rest == 0) break;
            const void* W = lp.FullTriangle(lower, unit, k0, kb);
            if (lower) {
                lp.Assign(k0, K0, kb, p, kb, -1.0, false, W, kb, false, lp.at(k0, K0), lp.ld);
                if (p > 0 && rest > 0)
                    exec::Gemm(lp.dev, lp.t, false, false, rest, p, kb, 1.0, lp.at(k1, k0), lp.ld, lp.at(k0, K0), lp.ld,
                               1.0, lp.at(k1, K0), lp.ld, lp.s);
                lp.Assign(k1, k0, rest, kb, kb, 1.0, false, lp.at(k1, k0), lp.ld, false, W, kb);
            } else {
                lp.Assign(K0, k0, p, kb, kb, -1.0, false, lp.at(K0, k0), lp.ld, false, W, kb);
                if (p > 0 && rest > 0)
                    exec::Gemm(lp.dev, lp.t, false, false, p, rest, kb, 1.0, lp.at(K0, k0), lp.ld, lp.at(k0, k1), lp.ld,
                               1.0, lp.at(K0, k1), lp.ld, lp.s);
                lp.Assign(k0, k1, kb, rest, kb, 1.0, false, W, kb, false, lp.at(k0, k1), lp.ld);
            }
        }
    };
    if (A.Height() > 0) sp.run(0, A.Height());
}

// On A in [MC,MR].  L^T L = [L11^T L11 + L21^T L21, .; L22^T L21, L22^T L22]
// (U U^T = [U11 U11^T + U12 U12^T, U12 U22^T; ., U22 U22^T]), the reference's
// panel operations (Trtrmm/LVar1.hpp, UVar1.hpp) split recursively: block 11
// is finished before the Syrk adds into it, and block 22 multiplies the
// off-diagonal block before it is overwritten.
void TrtrmmMCMR(bool lower, DistMatrix& A) {
    Split sp{A, LeafRows()};
    sp.kernel = [&](DistMatrix& a11, Int kb) {
        exec::Trtrmm(A.Dev(), A.Type(), lower, kb, a11.Buffer(), std::max<Int>(1, a11.LDim()), a11.Stream());
    };
    sp.mid = [&](Int k0, Int cut, Int k1) {
        auto A11 = DistMatrix::View(A, k0, cut, k0, cut);
        auto A22 = DistMatrix::View(A, cut, k1, cut, k1);
        if (lower) {
            auto A21 = DistMatrix::View(A, cut, k1, k0, cut);
            Syrk(ELX_LOWER, ELX_TRANSPOSE, 1.0, *A21, 1.0, *A11);
            Trmm(ELX_LEFT, ELX_LOWER, ELX_TRANSPOSE, ELX_NON_UNIT, 1.0, *A22, *A21);
        } else {
            auto A12 = DistMatrix::View(A, k0, cut, cut, k1);
            Syrk(ELX_UPPER, ELX_NORMAL, 1.0, *A12, 1.0, *A11);
            Trmm(ELX_RIGHT, ELX_UPPER, ELX_TRANSPOSE, ELX_NON_UNIT, 1.0, *A22, *A12);
        }
    };
    // trtrmm::LVar1 / UVar1 (LVar1.hpp:23-37) on A(K0:K1, K0:K1), one leaf per step,
    // with W = the diagonal block as a full matrix in place of the Trmm call:
    //   lower: L00 += L10^T L10 (triangle);  L10 := W^T L10;  L11 := L11^T L11
    //   upper: U00 += U01 U01^T (triangle);  U01 := U01 W^T;  U11 := U11 U11^T
    LocalPanels lp{A, sp.sweep_rows * sp.nb};
    sp.sweep = [&](Int K0, Int K1) {
        for (Int k0 = K0; k0 < K1; k0 += sp.nb) {
            const Int k1 = std::min(K1, k0 + sp.nb), kb = k1 - k0, p = k0 - K0;
            if (p > 0) {
                auto A00 = DistMatrix::View(A, K0, k0, K0, k0);
                const void* W = lp.FullTriangle(lower, false, k0, kb);
                if (lower) {
                    TrrkLocal(true, true, false, kb, 1.0, lp.at(k0, K0), lp.ld, lp.at(k0, K0), lp.ld, *A00, lp.s, lp.ttmp);
                    lp.Assign(k0, K0, kb, p, kb, 1.0, true, W, kb, false, lp.at(k0, K0), lp.ld);
                } else {
                    TrrkLocal(false, false, true, kb, 1.0, lp.at(K0, k0), lp.ld, lp.at(K0, k0), lp.ld, *A00, lp.s, lp.ttmp);
                    lp.Assign(K0, k0, p, kb, kb, 1.0, false, lp.at(K0, k0), lp.ld, true, W, kb);
                }
            }
            exec::Trtrmm(lp.dev, lp.t, lower, kb, lp.at(k0, k0), lp.ld, lp.s);
        }
    };
    if (A.Height() > 0) sp.run(0, A.Height());
}

}  // namespace

// TriangularInverse (src/lapack_like/funcs/Inverse/Triangular.cpp:48-54): A :=
// tri(A)^-1 in place on the uplo triangle; the other triangle, and with UNIT the
// diagonal, is neither read nor written.  No singularity test, as in the
// reference.  f64/f32.
void TriangularInverse(int uplo, int diag, DistMatrix& APre) {
    ELX_TRACE("El::TriangularInverse");
    ELX_REQUIRE(uplo == ELX_LOWER || uplo == ELX_UPPER, "TriangularInverse: bad UpperOrLower ", uplo);
    ELX_REQUIRE(diag == ELX_NON_UNIT || diag == ELX_UNIT, "TriangularInverse: bad UnitOrNonUnit ", diag);
    RequireSquareReal(APre, "TriangularInverse");
    RWProxy Ap(APre);
    TriangularInverseMCMR(uplo == ELX_LOWER, diag, Ap.Get());
    Ap.Finish();
}

// Trtrmm (src/blas_like/level3/Trtrmm.cpp): A := L^T L (LOWER) / U U^T (UPPER)
// in place on the uplo triangle.  Real types: `conjugate` changes nothing.
void Trtrmm(int uplo, DistMatrix& APre, bool /*conjugate*/) {
    ELX_TRACE("El::Trtrmm");
    ELX_REQUIRE(uplo == ELX_LOWER || uplo == ELX_UPPER, "Trtrmm: bad UpperOrLower ", uplo);
    RequireSquareReal(APre, "Trtrmm");
    RWProxy Ap(APre);
    TrtrmmMCMR(uplo == ELX_LOWER, Ap.Get());
    Ap.Finish();
}

// HPDInverse (src/lapack_like/funcs/Inverse/HPD.cpp): A := A^-1 on the uplo
// triangle as factor, invert the triangle, multiply it by its transpose
// (A^-1 = L^-T L^-1 = U^-1 U^-T).  The reference fuses the three into one sweep
// (HPD/CholeskyLVar2.hpp); the result is the same matrix to rounding.
// NonHPDMatrixError comes out of the first stage on every rank.
void HPDInverse(int uplo, DistMatrix& APre) {
    ELX_TRACE("El::HPDInverse");
    ELX_REQUIRE(uplo == ELX_LOWER || uplo == ELX_UPPER, "HPDInverse: bad UpperOrLower ", uplo);
    RequireSquareReal(APre, "HPDInverse");
    RWProxy Ap(APre);
    DistMatrix& A = Ap.Get();
    Cholesky(uplo, A);
    TriangularInverseMCMR(uplo == ELX_LOWER, ELX_NON_UNIT, A);
    TrtrmmMCMR(uplo == ELX_LOWER, A);
    Ap.Finish();
}

}  // namespace elx
