// El::Cholesky and cholesky::SolveAfter on DistMatrices.
#include "level3_internal.hpp"
#include <cstdlib>
#include "exec.hpp"
#include <algorithm>
#include <functional>
#include "../runtime/trace.hpp"

namespace elx {

using namespace detail;

// Cholesky on a DistMatrix (src/lapack_like/factor/Cholesky/LowerVariant3.hpp:
// 78-134 and UpperVariant3.hpp): A = L L^T (LOWER) or U^T U (UPPER) in place on
// the uplo triangle; the other triangle is neither read nor written.  The
// reference sweeps nb columns at a time (factor A11, solve the panel under it,
// update all of A22 with k = nb).  Here the same three steps are split
// recursively at block boundaries, as TrsmLeft is:
//   factor A11 (recursion);  A21 := A21 L11^-T (Trsm);  A22 -= A21 A21^T (Syrk);
//   factor A22 (recursion)
// so half of the update FLOPs run as one k = n/2 Syrk, a quarter as two k = n/4
// ones, ...  A leaf is one diagonal block of at most min(Blocksize(),
// kPotrfMax) rows: A11[*,*] <- A11, factored redundantly on every rank
// (potrf_kernel on the GPU), A11 <- A11[*,*]; in place where the local storage
// already is the [*,*] layout (1x1 grid).  One info word lives for the whole
// call: a leaf whose pivot is not > 0 records the 1-based column, later leaves
// see it and do nothing, and it is read back once after the last leaf; every
// rank factors the same leaves, so all ranks throw NonHPDMatrixError together.
// ELX_CHOLESKY_FLAT=1: the reference's flat nb-step order (ablation).  f64/f32.
void Cholesky(int uplo, DistMatrix& APre) {
    ELX_TRACE("El::Cholesky");
    ELX_REQUIRE(uplo == ELX_LOWER || uplo == ELX_UPPER, "Cholesky: bad UpperOrLower ", uplo);
    if (APre.Height() != APre.Width()) throw LogicError("A must be square");
    RequireReal(APre.Type(), "Cholesky");
    RWProxy Ap(APre);
    DistMatrix& A = Ap.Get();
    const Int n = A.Height();
    const bool lower = uplo == ELX_LOWER, gpu = A.Dev() == Device::GPU;
    const Int nb = std::max<Int>(1, std::min<Int>(Blocksize(), kern::kPotrfMax));
    int info_host = 0;
    int* info = &info_host;
    Buffer info_dev;
    if (gpu) {
        info_dev.Reset(Device::GPU, sizeof(int), A.Stream());
        info = static_cast<int*>(info_dev.data());
        ELX_CHECK_HIP(hipMemsetAsync(info, 0, sizeof(int), A.Stream()));
    }
    auto A11s = A.Like(Dist::STAR, Dist::STAR);
    auto leaf = [&](Int k0, Int k1) {
        auto A11 = DistMatrix::View(A, k0, k1, k0, k1);
        DistMatrix& a11 = StageDiagonalBlock(*A11, *A11s);
        exec::Cholesky(A.Dev(), A.Type(), lower, k1 - k0, a11.Buffer(), std::max<Int>(1, a11.LDim()), info,
                       static_cast<int>(k0), a11.Stream());
        if (&a11 != A11.get()) Copy(a11, *A11);              // A11[MC,MR] <- A11[*,*]
    };
    // the panel beside A(k0:mid, k0:mid) and the trailing block A(mid:k1, mid:k1)
    auto eliminate = [&](Int k0, Int mid, Int k1) {
        auto A11 = DistMatrix::View(A, k0, mid, k0, mid);
        auto A22 = DistMatrix::View(A, mid, k1, mid, k1);
        if (lower) {
            auto A21 = DistMatrix::View(A, mid, k1, k0, mid);
            Trsm(ELX_RIGHT, ELX_LOWER, ELX_TRANSPOSE, ELX_NON_UNIT, 1.0, *A11, *A21);
            Syrk(ELX_LOWER, ELX_NORMAL, -1.0, *A21, 1.0, *A22);
        } else {
            auto A12 = DistMatrix::View(A, k0, mid, mid, k1);
            Trsm(ELX_LEFT, ELX_UPPER, ELX_TRANSPOSE, ELX_NON_UNIT, 1.0, *A11, *A12);
            Syrk(ELX_UPPER, ELX_TRANSPOSE, -1.0, *A12, 1.0, *A22);
        }
    };
    // A whose local block is the whole matrix on the GPU (1x1 grid): the recursion
    // stops at blocks of ELX_CHOLESKY_SWEEP rows (default 1024; 0: recurse down to
    // single leaves; read per call, for A/B) and sweeps such a block leaf by leaf
    // with direct launches on the local buffer: potrf leaf, op(A11)^-T from the
    // batched inverse kernel, the panel as one MFMA GEMM with it, the trailing
    // triangle through TrrkLocal.  The same eliminations, but six launches per
    // leaf instead of a Trsm and a Syrk call on views (proxies, transposes and
    // pipeline set-up: ~0.4 ms of host time per leaf, which made the run time
    // linear in n: profiles/cholesky_bench.log).
    const char* sweep_s = getenv("ELX_CHOLESKY_SWEEP");
    const bool local = gpu && SameLocalLayout(A, Dist::STAR, Dist::STAR, 0, 0) && A.LocalHeight() == n &&
                       A.LocalWidth() == n && A.LDim() > 0 &&
                       kern::tri_inverse_lds_ok(static_cast<int>(A.Type()), nb);
    const Int sweep_rows = local ? (sweep_s ? (Int)atoll(sweep_s) : (Int)1024) : 0;
    Buffer winv, ybuf, ttmp;
    auto sweep = [&](Int K0, Int K1) {
        const DType t = A.Type();
        const size_t es = DTypeSize(t);
        const Int ld = A.LDim();
        hipStream_t s = A.Stream();
        auto at = [&](Int i, Int j) { return static_cast<char*>(A.Buffer()) + (i + j * ld) * es; };
        for (Int k0 = K0; k0 < K1; k0 += nb) {
            const Int k1 = std::min(K1, k0 + nb), kb = k1 - k0, rest = K1 - k1;
            exec::Cholesky(Device::GPU, t, lower, kb, at(k0, k0), ld, info, static_cast<int>(k0), s);
            if (rest == 0) break;
            if (winv.bytes() < static_cast<size_t>(kb * kb) * es) winv.Reset(Device::GPU, nb * nb * es, s);
            if (ybuf.bytes() < static_cast<size_t>(rest * kb) * es) ybuf.Reset(Device::GPU, (K1 - K0) * nb * es, s);
            // W := op(A11)^-1 with op = transpose: L11^-T (lower) / U11^-T (upper)
            exec::TriInverseBatched(t, lower, true, false, kb, kb, at(k0, k0), ld, winv.data(), s);
            char* panel = lower ? at(k1, k0) : at(k0, k1);
            if (lower) {  // A21 := A21 L11^-T
                exec::Gemm(Device::GPU, t, false, false, rest, kb, kb, 1.0, panel, ld, winv.data(), kb, 0.0, ybuf.data(),
                           rest, s);
                const kern::Copy2D back{rest, kb, ybuf.data(), 1, rest, panel, 1, ld};
                exec::Copy2DBatch(Device::GPU, t, &back, 1, false, 0.0, s);
            } else {      // A12 := U11^-T A12
                exec::Gemm(Device::GPU, t, false, false, kb, rest, kb, 1.0, winv.data(), kb, panel, ld, 0.0, ybuf.data(),
                           kb, s);
                const kern::Copy2D back{kb, rest, ybuf.data(), 1, kb, panel, 1, ld};
                exec::Copy2DBatch(Device::GPU, t, &back, 1, false, 0.0, s);
            }
            // A22 -= A21 A21^T (lower) / A12^T A12 (upper), on A22's uplo triangle only
            auto A22 = DistMatrix::View(A, k1, K1, k1, K1);
            TrrkLocal(lower, !lower, lower, kb, -1.0, panel, ld, panel, ld, *A22, s, ttmp);
        }
    };
    const char* flat_s = getenv("ELX_CHOLESKY_FLAT");  // read per call, for A/B
    const bool flat = flat_s && atoi(flat_s) > 0;
    if (flat) {
        for (Int k0 = 0; k0 < n; k0 += nb) {
            const Int k1 = std::min(n, k0 + nb);
            leaf(k0, k1);
            if (k1 < n) eliminate(k0, k1, n);
        }
    } else {
        std::function<void(Int, Int)> factor = [&](Int K0, Int K1) {
            const Int nbk = (K1 - K0 + nb - 1) / nb;
            if (nbk <= 1) return leaf(K0, K1);
            if (K1 - K0 <= sweep_rows) return sweep(K0, K1);
            const Int mid = K0 + (nbk / 2) * nb;
            factor(K0, mid);
            eliminate(K0, mid, K1);
            factor(mid, K1);
        };
        if (n > 0) factor(0, n);
    }
    int column = info_host;
    if (gpu && n > 0) {
        ELX_CHECK_HIP(hipMemcpyAsync(&column, info, sizeof(int), hipMemcpyDeviceToHost, A.Stream()));
        ELX_CHECK_HIP(hipStreamSynchronize(A.Stream()));
    }
    if (column != 0) throw NonHPDMatrixError(column);
    Ap.Finish();
}

// cholesky::SolveAfter (src/lapack_like/factor/Cholesky/SolveAfter.hpp:78-107):
// B := A^-1 B from the factor A holds in its uplo triangle.  Real types: the
// orientation changes nothing (A is symmetric; the reference only conjugates B).
namespace cholesky {
void SolveAfter(int uplo, int orient, const DistMatrix& A, DistMatrix& B) {
    ELX_REQUIRE(uplo == ELX_LOWER || uplo == ELX_UPPER, "SolveAfter: bad UpperOrLower ", uplo);
    ELX_REQUIRE(orient >= ELX_NORMAL && orient <= ELX_ADJOINT, "SolveAfter: bad orientation");
    if (A.Height() != A.Width()) throw LogicError("A must be square");
    if (A.Height() != B.Height()) throw LogicError("A and B must be the same height");
    if (uplo == ELX_LOWER) {
        Trsm(ELX_LEFT, ELX_LOWER, ELX_NORMAL, ELX_NON_UNIT, 1.0, A, B);
        Trsm(ELX_LEFT, ELX_LOWER, ELX_TRANSPOSE, ELX_NON_UNIT, 1.0, A, B);
    } else {
        Trsm(ELX_LEFT, ELX_UPPER, ELX_TRANSPOSE, ELX_NON_UNIT, 1.0, A, B);
        Trsm(ELX_LEFT, ELX_UPPER, ELX_NORMAL, ELX_NON_UNIT, 1.0, A, B);
    }
}
}  // namespace cholesky

}  // namespace elx
