// The triangle drivers on DistMatrices, built on the C-stationary SUMMA
// pipeline of gemm.cpp: ScaleTrapezoid, Syrk, Trrk, Syr2k, Symm, Trsm, Trmm.
#include "level3_internal.hpp"
#include <cstdlib>
#include "exec.hpp"
#include <algorithm>
#include <functional>
#include "../runtime/trace.hpp"

namespace elx {

using namespace detail;

void ScaleTrapezoid(double alpha, int uplo, DistMatrix& A, Int offset) {
    ELX_REQUIRE(uplo == ELX_LOWER || uplo == ELX_UPPER, "ScaleTrapezoid: bad UpperOrLower ", uplo);
    if (alpha == 1.0) return;  // ScaleTrapezoid.hpp:52-53
    exec::Trapezoid(A.Dev(), A.Type(), uplo == ELX_LOWER, A.LocalHeight(), A.LocalWidth(), 0.0, nullptr, 0, alpha,
                    A.Buffer(), A.LDim(), A.ColShift(), A.ColStride(), A.RowShift(), A.RowStride(), offset,
                    A.Stream());
}

// Syrk / Herk on DistMatrices (src/blas_like/level3/Syrk.cpp:196-211): the
// trapezoid of C is scaled by beta, then LN/LT/UN/UT run as the C-stationary
// pipeline with the triangular local update (Syrk/LN.hpp:13-48 and siblings:
// A1[MC,*] and A1^T[*,MR] per panel, LocalTrrk).  Real types only, so the
// conjugate flag (Herk) changes nothing.  The reference switches to its Dot
// variant when width > 10 height (LN.hpp:156); here the panel pipeline serves
// every shape (same sums, summation order within the normwise tolerance).
void Syrk(int uplo, int orient, double alpha, const DistMatrix& A, double beta, DistMatrix& C) {
    ELX_TRACE("El::Syrk");
    ELX_REQUIRE(uplo == ELX_LOWER || uplo == ELX_UPPER, "Syrk: bad UpperOrLower ", uplo);
    ELX_REQUIRE(orient >= ELX_NORMAL && orient <= ELX_ADJOINT, "Syrk: bad orientation");
    ELX_REQUIRE(&A.G() == &C.G(), "Syrk: matrices on different grids");
    ELX_REQUIRE(A.Type() == C.Type(), "Syrk: mixed types");
    const bool N = orient == ELX_NORMAL;
    const Int n = N ? A.Height() : A.Width();
    if (C.Height() != n || C.Width() != n) throw LogicError("Nonconformal Syrk");
    ScaleTrapezoid(beta, uplo, C, 0);
    if (N) SummaC(ELX_NORMAL, ELX_TRANSPOSE, alpha, A, A, 1.0, C, uplo);
    else SummaC(ELX_TRANSPOSE, ELX_NORMAL, alpha, A, A, 1.0, C, uplo);
}

// Trrk on DistMatrices (src/blas_like/level3/Trrk.cpp:100-117): C := alpha op(A)
// op(B) + beta C on C's uplo triangle; TrrkNN/NT/TN/TT are the same C-stationary
// pipeline with the triangular local update.
void Trrk(int uplo, int oA, int oB, double alpha, const DistMatrix& A, const DistMatrix& B, double beta,
          DistMatrix& C) {
    ELX_REQUIRE(uplo == ELX_LOWER || uplo == ELX_UPPER, "Trrk: bad UpperOrLower ", uplo);
    ELX_REQUIRE(&A.G() == &B.G() && &A.G() == &C.G(), "Trrk: matrices on different grids");
    ELX_REQUIRE(A.Type() == B.Type() && A.Type() == C.Type(), "Trrk: mixed types");
    if (oA == ELX_ADJOINT) oA = ELX_TRANSPOSE;
    if (oB == ELX_ADJOINT) oB = ELX_TRANSPOSE;
    const Int m = IsN(oA) ? A.Height() : A.Width(), k = IsN(oA) ? A.Width() : A.Height();
    const Int kb = IsN(oB) ? B.Height() : B.Width(), n = IsN(oB) ? B.Width() : B.Height();
    if (m != C.Height() || n != C.Width() || k != kb || m != n) throw LogicError("Nonconformal Trrk");
    ScaleTrapezoid(beta, uplo, C, 0);
    SummaC(oA, oB, alpha, A, B, 1.0, C, uplo);
}

// Syr2k / Her2k (src/blas_like/level3/Syr2k.cpp:78-93, Syr2k/LN.hpp): C := alpha
// (op(A) op(B)^T + op(B) op(A)^T) + beta C on C's uplo triangle.  The reference
// gathers both panels and runs two LocalTrrks per panel; here each term is one
// pass of the triangular pipeline.  Real types: conj(alpha) = alpha.
void Syr2k(int uplo, int orient, double alpha, const DistMatrix& A, const DistMatrix& B, double beta,
           DistMatrix& C) {
    ELX_REQUIRE(uplo == ELX_LOWER || uplo == ELX_UPPER, "Syr2k: bad UpperOrLower ", uplo);
    ELX_REQUIRE(orient >= ELX_NORMAL && orient <= ELX_ADJOINT, "Syr2k: bad orientation");
    ELX_REQUIRE(&A.G() == &B.G() && &A.G() == &C.G(), "Syr2k: matrices on different grids");
    ELX_REQUIRE(A.Type() == B.Type() && A.Type() == C.Type(), "Syr2k: mixed types");
    const bool N = orient == ELX_NORMAL;
    const Int n = N ? A.Height() : A.Width();
    if (A.Height() != B.Height() || A.Width() != B.Width() || C.Height() != n || C.Width() != n)
        throw LogicError("Nonconformal Syr2k");
    ScaleTrapezoid(beta, uplo, C, 0);
    const int oA = N ? ELX_NORMAL : ELX_TRANSPOSE, oB = N ? ELX_TRANSPOSE : ELX_NORMAL;
    SummaC(oA, oB, alpha, A, B, 1.0, C, uplo);
    SummaC(oA, oB, alpha, B, A, 1.0, C, uplo);
}

DistMatrix& detail::StageDiagonalBlock(DistMatrix& A11, DistMatrix& stage) {
    if (SameLocalLayout(A11, Dist::STAR, Dist::STAR, 0, 0)) return A11;
    Copy(A11, stage);                                    // A11[*,*] <- A11[MC,MR]
    return stage;
}

namespace {
// What TrsmLeft and TrmmLeft share: the operands of an in-place sweep over the
// diagonal blocks of op(tri(A)) (m x m) applied to X (m x n) from the left, the
// update between blocks and the staging of one block for a local kernel.
struct LeftSweep {
    MultiSync sync;
    std::shared_ptr<const DistMatrix> Ap;
    RWProxy Xp;
    const DistMatrix& A;                    // [MC,MR] on X's device and stream
    DistMatrix& X;                          // [MC,MR]; Xp.Finish() copies it back
    const Int m, n;
    const bool trans, lower, op_lower;      // op_lower: op(A) is lower triangular
    std::shared_ptr<DistMatrix> A11s, X1v;  // the leaves' [*,*] / [*,VR] staging, one pair per call
    LeftSweep(int uplo, int orient, const DistMatrix& APre, DistMatrix& XPre)
        : sync(XPre.Stream(), {APre.Stream()}), Ap(ReadProxy(APre, XPre, Dist::MC, Dist::MR)), Xp(XPre), A(*Ap),
          X(Xp.Get()), m(X.Height()), n(X.Width()), trans(orient != ELX_NORMAL), lower(uplo == ELX_LOWER),
          op_lower(lower != trans), A11s(A.Like(Dist::STAR, Dist::STAR)), X1v(X.Like(Dist::STAR, Dist::VR)) {}

    // X(r0:r1, :) += alpha op(A)(r0:r1, k0:k1) src(k0:k1, :): the SUMMA pipeline on
    // views, or (local: every operand's local block is the whole matrix) one MFMA
    // GEMM on the local buffers, no views, proxies or pipeline on the host
    void Update(double alpha, Int r0, Int r1, Int k0, Int k1, const DistMatrix& src, bool local) {
        if (r1 <= r0 || k1 <= k0 || n == 0) return;
        if (local) {
            const size_t es = DTypeSize(X.Type());
            const char* a = static_cast<const char*>(A.Buffer()) +
                            ((trans ? k0 + r0 * A.LDim() : r0 + k0 * A.LDim()) * es);
            const char* xk = static_cast<const char*>(src.Buffer()) + k0 * es;
            char* xr = static_cast<char*>(X.Buffer()) + r0 * es;
            exec::Gemm(X.Dev(), X.Type(), trans, false, r1 - r0, n, k1 - k0, alpha, a, A.LDim(), xk, src.LDim(), 1.0,
                       xr, X.LDim(), X.Stream());
            return;
        }
        auto Ar = trans ? DistMatrix::View(A, k0, k1, r0, r1) : DistMatrix::View(A, r0, r1, k0, k1);
        auto Xk = DistMatrix::View(src, k0, k1, 0, n);
        auto Xr = DistMatrix::View(X, r0, r1, 0, n);
        SummaC(trans ? ELX_TRANSPOSE : ELX_NORMAL, ELX_NORMAL, alpha, *Ar, *Xk, 1.0, *Xr);
    }
    // One diagonal block: fn(a11, x1) with A11 as [*,*] and X1 = X(k0:k1, :) as
    // [*,VR], ordered on x1's stream; X1 is copied back afterwards.  A block whose
    // local storage already IS that layout (a 1x1 grid) is used in place.
    template <class Fn>
    void WithLeafBlocks(Int k0, Int k1, Fn fn) {
        auto X1 = DistMatrix::View(X, k0, k1, 0, n);
        auto A11 = DistMatrix::View(A, k0, k1, k0, k1);
        const DistMatrix& a11 = StageDiagonalBlock(*A11, *A11s);
        const bool inplace = SameLocalLayout(*X1, Dist::STAR, Dist::VR, 0, X1->RowAlign());
        DistMatrix* x1 = X1.get();
        if (!inplace) {
            X1v->AlignRows(X.RowAlign(), true);
            Copy(*X1, *X1v);                                 // X1[*,VR] <- X1[MC,MR]
            x1 = X1v.get();
        }
        if (X.Dev() == Device::GPU) FenceStreams(a11.Stream(), x1->Stream());
        fn(a11, *x1);
        if (!inplace) Copy(*X1v, *X1);                       // X1[MC,MR] <- X1[*,VR]
    }
};

// Recursive split of rows [K0, K1) at an nb-block boundary: one half (the low
// one when low_first), couple(f0, f1, s0, s1) with [f0, f1) that half and
// [s0, s1) the other, then the other half; leaf(k0, k1) for a single block.  The
// same couplings as an nb-step sweep, but half of their FLOPs go to ONE GEMM of
// k = (K1 - K0) / 2, a quarter to two of half that, ...: deep, full-machine MFMA
// launches instead of (K1 - K0) / nb ones of k = nb.
void SplitBlocks(Int K0, Int K1, Int nb, bool low_first, const std::function<void(Int, Int)>& leaf,
                 const std::function<void(Int, Int, Int, Int)>& couple) {
    const Int nbk = (K1 - K0 + nb - 1) / nb;
    if (nbk <= 1) return leaf(K0, K1);
    const Int mid = K0 + (nbk / 2) * nb;
    const Int f0 = low_first ? K0 : mid, f1 = low_first ? mid : K1;
    const Int s0 = low_first ? mid : K0, s1 = low_first ? K1 : mid;
    SplitBlocks(f0, f1, nb, low_first, leaf, couple);
    couple(f0, f1, s0, s1);
    SplitBlocks(s0, s1, nb, low_first, leaf, couple);
}

// The front door of Trsm and Trmm: the argument checks (`name` prefixes the
// messages; not_square and nonconformal are the two that the reference words
// differently), Trsm's test for a singular A, B *= alpha, then the LEFT sweep;
// RIGHT as the transposed LEFT problem through two distributed transposes.
using LeftFn = void (*)(int uplo, int orient, bool unit, const DistMatrix& A, DistMatrix& X);
void TriangularFrontDoor(const char* name, const char* not_square, const char* nonconformal, LeftFn left, int side,
                         int uplo, int orient, int diag, double alpha, const DistMatrix& A, DistMatrix& B,
                         bool checkIfSingular) {
    ELX_REQUIRE(side == ELX_LEFT || side == ELX_RIGHT, name, ": bad LeftOrRight ", side);
    ELX_REQUIRE(uplo == ELX_LOWER || uplo == ELX_UPPER, name, ": bad UpperOrLower ", uplo);
    ELX_REQUIRE(orient >= ELX_NORMAL && orient <= ELX_ADJOINT, name, ": bad orientation");
    ELX_REQUIRE(diag == ELX_NON_UNIT || diag == ELX_UNIT, name, ": bad UnitOrNonUnit ", diag);
    ELX_REQUIRE(&A.G() == &B.G(), name, ": matrices on different grids");
    ELX_REQUIRE(A.Type() == B.Type(), name, ": mixed types");
    RequireReal(A.Type(), name);
    if (A.Height() != A.Width()) throw LogicError(not_square);  // Trsm.cpp:142-143, Trmm.cpp:31-32
    if ((side == ELX_LEFT ? B.Height() : B.Width()) != A.Height()) throw LogicError(nonconformal);
    if (checkIfSingular && diag != ELX_UNIT && DiagonalHasZero(A)) throw SingularMatrixError();
    Scale(alpha, B);  // Trsm.cpp:155, Trmm.cpp:60 (B *= alpha)
    if (side == ELX_LEFT) return left(uplo, orient, diag == ELX_UNIT, A, B);
    auto Bt = B.Like(Dist::MC, Dist::MR);
    Transpose(B, *Bt);  // B op(A) = (op(A)^T B^T)^T
    left(uplo, orient == ELX_NORMAL ? ELX_TRANSPOSE : ELX_NORMAL, diag == ELX_UNIT, A, *Bt);
    Transpose(*Bt, B);
}

// Trsm on DistMatrices (src/blas_like/level3/Trsm.cpp:129-420): B := alpha
// op(A)^-1 B (LEFT) or alpha B op(A)^-1 (RIGHT).  LEFT follows Trsm/LLN.hpp:40-70
// (and LUN/LLT/LUT with the block order reversed where op(A) is upper):
//   A11[*,*] <- A11;  X1[*,VR] <- X1;  X1[*,VR] := op(A11)^-1 X1 (trsm_kernel);
//   X1 <- X1[*,VR];   X_rest -= op(A)_rest,1 X1 (the C-stationary SUMMA on views:
//   op(A) panel gathered [MC,*] / [*,MC], X1 as [*,MR], MFMA update).
// RIGHT solves the transposed LEFT problem (X op(A) = B <=> op(A)^T X^T = B^T)
// through two distributed transposes.  f64/f32 (the reference's GPU Trsm types).
// ELX_TRSM_FLAT=1: the reference's flat nb-step sweep (every update k = nb over
// all remaining rows) instead of the recursive split (tests, ablation)
void TrsmLeft(int uplo, int orient, bool unit, const DistMatrix& APre, DistMatrix& XPre) {
    ELX_TRACE("El::Trsm");
    LeftSweep S(uplo, orient, APre, XPre);
    const DistMatrix& A = S.A;
    DistMatrix& X = S.X;
    const Int m = S.m, n = S.n;
    Int nb = std::max<Int>(1, Blocksize());
    const bool forward = S.op_lower;  // op(A) lower: blocks top to bottom
    // A whose local block is the whole matrix (1x1 grid): every diagonal block's
    // inverse comes from ONE batched launch up front (the per-block inversions
    // are independent), applied per block as an MFMA GEMM whose output goes
    // straight into a second buffer Y (no write-back per block; every later
    // update reads solved rows from Y, copied into X once at the end);
    // elsewhere each block is solved where it lands (exec::Trsm)
    const size_t es = DTypeSize(X.Type());
    Buffer winv;
    auto batch_ok = [&](Int b) {
        return X.Dev() == Device::GPU && SameLocalLayout(A, Dist::STAR, Dist::STAR, 0, 0) &&
               SameLocalLayout(X, Dist::STAR, Dist::VR, 0, X.RowAlign()) &&
               kern::trsm_batched_ok(es, b, m, X.LocalWidth()) &&
               kern::tri_inverse_lds_ok(static_cast<int>(X.Type()), b);
    };
    // Batched path with the default Blocksize (128) and a large system: 256-row
    // diagonal blocks, so every leaf (inverse applied as a GEMM) and the lowest
    // updates are 256 x n MFMA launches (256 output tiles, the whole machine)
    // instead of 128 x n ones (half of it); ELX_TRSM_NB256=0 keeps 128.
    static const bool nb256 = [] { const char* e = getenv("ELX_TRSM_NB256"); return !e || atoi(e) != 0; }();
    if (nb256 && nb == 128 && m >= 8 * 256 && batch_ok(256)) nb = 256;
    const bool batched = batch_ok(nb);
    std::shared_ptr<DistMatrix> Y;
    const DistMatrix* src = &X;  // where updates read solved rows: X itself, or Y on the batched path
    bool local = false;          // set on the batched path: every operand's local block is the whole matrix
    if (batched) {
        FenceStreams(A.Stream(), X.Stream());
        winv.Reset(Device::GPU, static_cast<size_t>((m + nb - 1) / nb) * nb * nb * es, X.Stream());
        exec::TriInverseBatched(X.Type(), S.lower, S.trans, unit, nb, m, A.Buffer(), A.LDim(), winv.data(),
                                X.Stream());
        Y = X.Like(Dist::MC, Dist::MR);
        Y->Align(X.ColAlign(), X.RowAlign(), true);
        Y->Resize(m, n);
        src = Y.get();
        local = X.LocalHeight() == m && X.LocalWidth() == n && Y->LDim() > 0 && !getenv("ELX_TRSM_SUMMA");
    }
    // X_rest(r0:r1, :) -= op(A)(r0:r1, k0:k1) X(k0:k1, :)
    auto update = [&](Int r0, Int r1, Int k0, Int k1) { S.Update(-1.0, r0, r1, k0, k1, *src, local); };
    // X(k0:k1, :) := op(A11)^-1 X(k0:k1, :), one nb block (Trsm/LLN.hpp:49-60)
    auto leaf = [&](Int k0, Int k1) {
        if (batched) {
            auto X1 = DistMatrix::View(X, k0, k1, 0, n);
            auto Y1 = DistMatrix::View(*Y, k0, k1, 0, n);
            exec::Gemm(X.Dev(), X.Type(), false, false, k1 - k0, X1->LocalWidth(), k1 - k0, 1.0,
                       static_cast<const char*>(winv.data()) + (k0 / nb) * nb * nb * es, nb, X1->Buffer(),
                       X1->LDim(), 0.0, Y1->Buffer(), Y1->LDim(), X1->Stream());
            return;
        }
        S.WithLeafBlocks(k0, k1, [&](const DistMatrix& a11, DistMatrix& x1) {
            exec::Trsm(X.Dev(), X.Type(), S.lower, S.trans, unit, k1 - k0, x1.LocalWidth(), a11.Buffer(), a11.LDim(),
                       x1.Buffer(), x1.LDim(), x1.Stream());
        });
    };
    static const bool flat = [] { const char* e = getenv("ELX_TRSM_FLAT"); return e && atoi(e) > 0; }();
    if (flat) {
        // the reference's order (Trsm/LLN.hpp:40-70): solve block b, then update
        // every remaining row with k = nb
        const Int nblk = (m + nb - 1) / nb;
        for (Int bi = 0; bi < nblk; ++bi) {
            const Int b = forward ? bi : nblk - 1 - bi;
            const Int k0 = b * nb, k1 = std::min(m, k0 + nb);
            leaf(k0, k1);
            if (forward) update(k1, m, k0, k1);
            else update(0, k0, k0, k1);
        }
    } else if (m > 0) {
        // solve the half op(A) reaches first, eliminate it from the other half
        // with ONE GEMM (k = that half's height), solve the other half
        SplitBlocks(0, m, nb, forward, leaf, [&](Int f0, Int f1, Int s0, Int s1) { update(s0, s1, f0, f1); });
    }
    if (Y) Copy(*Y, X);
    S.Xp.Finish();
}

// Trmm on DistMatrices (src/blas_like/level3/Trmm.cpp:53-89): B := alpha
// op(tri(A)) B (LEFT) or alpha B op(tri(A)) (RIGHT), in place.  LEFT is the
// reference's LLNC / LUNC sweep (Trmm/LLN.hpp:178-228) in the order that never
// overwrites rows still to be read, split recursively at block boundaries as
// TrsmLeft is: with op(A) lower,
//   X[mid:K1] := op(A)[mid:K1, mid:K1] X[mid:K1]       (recursion)
//   X[mid:K1] += op(A)[mid:K1, K0:mid] X[K0:mid]       (C-stationary SUMMA on views)
//   X[K0:mid] := op(A)[K0:mid, K0:mid] X[K0:mid]       (recursion)
// and mirrored with op(A) upper.  A leaf is one diagonal block: A11[*,*] <- A11,
// X1[*,VR] <- X1, X1 := op(tri(A11)) X1 (trmm_tile_kernel, which skips the zero
// half of A11), X1 <- X1[*,VR].  RIGHT runs the transposed LEFT problem through
// two distributed transposes, as Trsm does.  f64/f32.
void TrmmLeft(int uplo, int orient, bool unit, const DistMatrix& APre, DistMatrix& XPre) {
    ELX_TRACE("El::Trmm");
    LeftSweep S(uplo, orient, APre, XPre);
    const DistMatrix& A = S.A;
    DistMatrix& X = S.X;
    const Int m = S.m, n = S.n;
    Int nb = std::max<Int>(1, Blocksize());
    // every operand's local block is the whole matrix (1x1 grid): updates are
    // direct MFMA GEMMs on the local buffers, no views, proxies or pipeline
    const bool local = SameLocalLayout(A, Dist::STAR, Dist::STAR, 0, 0) &&
                       SameLocalLayout(X, Dist::STAR, Dist::VR, 0, X.RowAlign()) && X.LocalHeight() == m &&
                       X.LocalWidth() == n && X.LDim() > 0;
    // There, with the default Blocksize (128) on the GPU, the leaf is widened to
    // ELX_TRMM_LEAF rows (default 512; 0 keeps the blocksize) once the matrix
    // holds two of them: one triangle-aware launch that fills the chip instead
    // of a cascade of 128-row leaves and k = 128, 256, ... updates (read per
    // call, for A/B)
    const char* leaf_s = getenv("ELX_TRMM_LEAF");
    const Int leaf_env = leaf_s ? (Int)atoll(leaf_s) : (Int)512;
    if (local && X.Dev() == Device::GPU && nb == 128 && leaf_env > nb && m >= 2 * leaf_env) nb = leaf_env;
    if (local && X.Dev() == Device::GPU) FenceStreams(A.Stream(), X.Stream());
    // X(k0:k1, :) := op(tri(A11)) X(k0:k1, :), one diagonal block
    auto leaf = [&](Int k0, Int k1) {
        S.WithLeafBlocks(k0, k1, [&](const DistMatrix& a11, DistMatrix& x1) {
            exec::Trmm(X.Dev(), X.Type(), S.lower, S.trans, unit, k1 - k0, x1.LocalWidth(), 1.0, a11.Buffer(),
                       a11.LDim(), x1.Buffer(), x1.LDim(), x1.Stream());
        });
    };
    // the half op(A) completes first, while the other half's rows are still
    // unmultiplied: X(f0:f1, :) += op(A)(f0:f1, s0:s1) X(s0:s1, :)
    if (m > 0 && n > 0)
        SplitBlocks(0, m, nb, !S.op_lower, leaf,
                    [&](Int f0, Int f1, Int s0, Int s1) { S.Update(1.0, f0, f1, s0, s1, X, local); });
    S.Xp.Finish();
}

}  // namespace

void Trsm(int side, int uplo, int orient, int diag, double alpha, const DistMatrix& A, DistMatrix& B,
          bool checkIfSingular) {
    TriangularFrontDoor("Trsm", "A must be square", "Nonconformal Trsm", TrsmLeft, side, uplo, orient, diag, alpha, A,
                        B, checkIfSingular);
}

void Trmm(int side, int uplo, int orient, int diag, double alpha, const DistMatrix& A, DistMatrix& B) {
    TriangularFrontDoor("Trmm", "Triangular matrix must be square", "Nonconformal Trmm", TrmmLeft, side, uplo, orient,
                        diag, alpha, A, B, false);
}

// Symm / Hemm on DistMatrices (src/blas_like/level3/Symm.cpp:55-80): C := alpha
// A B + beta C (LEFT) or alpha B A + beta C (RIGHT), A symmetric with only its
// uplo triangle read.  The reference accumulates triangle-aware local products
// (Symm/LL.hpp LocalAccumulateLL); here A is completed once into a full [MC,MR]
// copy (one distributed transpose + a trapezoid copy of the mirrored strict
// triangle, O(n^2) HBM work) and the product runs through El::Gemm's pipeline.
void Symm(int side, int uplo, double alpha, const DistMatrix& A, const DistMatrix& B, double beta, DistMatrix& C) {
    ELX_REQUIRE(side == ELX_LEFT || side == ELX_RIGHT, "Symm: bad LeftOrRight ", side);
    ELX_REQUIRE(uplo == ELX_LOWER || uplo == ELX_UPPER, "Symm: bad UpperOrLower ", uplo);
    ELX_REQUIRE(&A.G() == &B.G() && &A.G() == &C.G(), "Symm: matrices on different grids");
    ELX_REQUIRE(A.Type() == B.Type() && A.Type() == C.Type(), "Symm: mixed types");
    if (A.Height() != A.Width()) throw LogicError("A must be square");
    const bool left = side == ELX_LEFT;
    if ((left ? B.Height() : B.Width()) != A.Height() || C.Height() != B.Height() || C.Width() != B.Width())
        throw LogicError("Nonconformal Symm");
    auto S = A.Like(Dist::MC, Dist::MR);
    Copy(A, *S);
    auto T = A.Like(Dist::MC, Dist::MR);
    T->AlignWith(*S, true);
    Transpose(*S, *T);
    // S's strictly-other triangle := T's (lower stored: strict upper is gi <= gj - 1)
    const bool other_lower = uplo == ELX_UPPER;
    if (S->Dev() == Device::GPU) FenceStreams(T->Stream(), S->Stream());
    exec::Trapezoid(S->Dev(), S->Type(), other_lower, S->LocalHeight(), S->LocalWidth(), 1.0, T->Buffer(), T->LDim(),
                    0.0, S->Buffer(), S->LDim(), S->ColShift(), S->ColStride(), S->RowShift(), S->RowStride(),
                    other_lower ? -1 : 1, S->Stream());
    if (left) Gemm(ELX_NORMAL, ELX_NORMAL, alpha, *S, B, beta, C, ELX_GEMM_DEFAULT);
    else Gemm(ELX_NORMAL, ELX_NORMAL, alpha, B, *S, beta, C, ELX_GEMM_DEFAULT);
}

}  // namespace elx
