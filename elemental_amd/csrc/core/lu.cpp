// El::LU with partial pivoting, lu::SolveAfter and LinearSolve.
#include "lu.hpp"
#include "level3_internal.hpp"
#include "exec.hpp"
#include "../runtime/trace.hpp"
#include <algorithm>
#include <functional>

namespace elx {

using namespace detail;

namespace {

// B := L^-1 B, L unit lower triangular m x m, B m x n, on the local buffers.  On the
// GPU a diagonal block of kTrsmBlock rows is solved by the in-LDS substitution
// kernel and the blocks are joined by the recursive split, one MFMA GEMM per join.
// Substitution, not a GEMM with the block's inverse: |L| <= 1 bounds L but not
// L^-1, and with inverted 64-row blocks the f32 forced-pivot test lost its pivots.
// Blocks of 64 rows, not exec::Trsm's up to 256: the kernel walks a dependent chain
// of m^2 / 2 steps per call and leaves LDS above 129 rows (f64); with 256-row
// blocks most of an n = 16384 factorization's kernel time was Trsm (seen in a
// trace while this was built; that trace is not kept in profiles/).
constexpr Int kTrsmBlock = 64;
void TrsmLowerUnit(Device dev, DType t, Int m, Int n, const char* L, Int ldl, char* B, Int ldb, hipStream_t s) {
    if (m <= 0 || n <= 0) return;
    if (dev == Device::CPU) return exec::Trsm(dev, t, true, false, true, m, n, L, ldl, B, ldb, s);
    const Int es = (Int)DTypeSize(t), nb = kTrsmBlock;
    std::function<void(Int, Int)> solve = [&](Int r0, Int r1) {
        const Int nbk = (r1 - r0 + nb - 1) / nb;
        if (nbk <= 1) {
            const hipError_t e = kern::trsm_local((int)t, false, true, false, true, r1 - r0, n, L + (r0 + r0 * ldl) * es,
                                                  ldl, B + r0 * es, ldb, s);
            if (e != hipSuccess) throw HIPError(Cat("trsm_local: ", hipGetErrorName(e)));
            return;
        }
        const Int mid = r0 + (nbk / 2) * nb;
        solve(r0, mid);
        exec::Gemm(dev, t, false, false, r1 - mid, n, mid - r0, -1.0, L + (mid + r0 * ldl) * es, ldl, B + r0 * es, ldb, 1.0,
                   B + mid * es, ldb, s);
        solve(mid, r1);
    };
    solve(0, m);
}

struct LocalLUCall {
    Device dev;
    DType t;
    Int m, ld, es;
    char* A;
    int* piv;  // piv[j]: col0 + the row swapped with row j
    int* info;
    void* work;
    int col0;
    hipStream_t s;
    char* at(Int i, Int j) const { return A + (i + j * ld) * es; }
    void Swap(Int k0, Int k1, Int c0, Int c1) const {  // the swaps k0..k1-1 on columns [c0, c1)
        exec::Laswp(dev, t, m, c1 - c0, at(0, c0), ld, piv, k0, k1, col0, false, info, s);
    }
    // P A = L U of A(c0:m, c0:c1) by recursion over columns (Toledo): the left half,
    // its swaps on the right half, A12 := L11^-1 A12, A22 -= A21 A12, the right
    // half, its swaps on the left half.  Direct launches on the buffer, one stream.
    void Factor(Int c0, Int c1) const {
        const Int n = c1 - c0;
        if (n <= kern::kGetrfLeafCols) {
            exec::LU(dev, t, m - c0, n, at(c0, c0), ld, piv + c0, col0 + (int)c0, work, info, col0 + (int)c0, s);
            return;
        }
        const Int L = kern::kGetrfLeafCols, cm = c0 + (n / 2 + L / 2) / L * L;
        Factor(c0, cm);
        Swap(c0, cm, cm, c1);
        TrsmLowerUnit(dev, t, cm - c0, c1 - cm, at(c0, c0), ld, at(c0, cm), ld, s);
        exec::Gemm(dev, t, false, false, m - cm, c1 - cm, cm - c0, -1.0, at(cm, c0), ld, at(c0, cm), ld, 1.0, at(cm, cm),
                   ld, s);
        Factor(cm, c1);
        Swap(cm, c1, c0, cm);
    }
};

}  // namespace

void LocalLU(Device dev, DType t, Int m, Int n, void* A, Int ld, int* piv, int* info, int col0, hipStream_t s) {
    RequireReal(t, "LU");
    const Int k = std::min(m, n);
    if (k <= 0) return;
    ELX_REQUIRE(ld >= m && piv && info, "LocalLU: bad arguments");
    Buffer work;  // the leaves' scratch, once per call
    if (exec::LUWorkBytes(dev, m) > 0) work.Reset(dev, exec::LUWorkBytes(dev, m), s);
    const LocalLUCall c{dev, t, m, ld, (Int)DTypeSize(t), static_cast<char*>(A), piv, info, work.data(), col0, s};
    c.Factor(0, k);
    if (n > m) {  // the columns right of the square part
        c.Swap(0, m, m, n);
        TrsmLowerUnit(dev, t, m, n - m, c.at(0, 0), ld, c.at(0, m), ld, s);
    }
}

void LU(DistMatrix& APre, Permutation& P) {
    ELX_TRACE("El::LU");
    RequireReal(APre.Type(), "LU");
    RWProxy Ap(APre);
    DistMatrix& A = Ap.Get();
    const Int m = A.Height(), n = A.Width(), k = std::min(m, n);
    const bool gpu = A.Dev() == Device::GPU;
    P.MakeIdentity(m, A.Dev(), gpu ? A.Stream() : nullptr);
    int* piv = P.Reserve(k);
    int info_host = 0;
    int* info = &info_host;
    Buffer info_dev;
    if (gpu) {
        info_dev.Reset(Device::GPU, sizeof(int), A.Stream());
        info = static_cast<int*>(info_dev.data());
        ELX_CHECK_HIP(hipMemsetAsync(info, 0, sizeof(int), A.Stream()));
    }
    const bool local = SameLocalLayout(A, Dist::STAR, Dist::STAR, 0, 0) && A.LocalHeight() == m && A.LocalWidth() == n;
    if (local) {
        LocalLU(A.Dev(), A.Type(), m, n, A.Buffer(), std::max<Int>(1, A.LDim()), piv, info, 0, A.Stream());
        P.SetNumSwaps(k, A.Stream());
    } else {
        // the reference's right-looking loop (LU.cpp:88-131): the panel A(k0:m, k0:k1)
        // factored redundantly on every rank as [*,*], its swaps on the columns left
        // and right of it, then A12 := L11^-1 A12 and A22 -= A21 A12 on views
        const Int nb = std::max<Int>(1, Blocksize());
        auto Ps = A.Like(Dist::STAR, Dist::STAR);
        for (Int k0 = 0; k0 < k; k0 += nb) {
            const Int k1 = std::min(k, k0 + nb);
            auto panel = DistMatrix::View(A, k0, m, k0, k1);
            Copy(*panel, *Ps);
            LocalLU(A.Dev(), A.Type(), m - k0, k1 - k0, Ps->Buffer(), std::max<Int>(1, Ps->LDim()), piv + k0, info,
                    (int)k0, Ps->Stream());
            Copy(*Ps, *panel);
            P.SetNumSwaps(k1, Ps->Stream());
            if (k0 > 0) P.PermuteRowsRange(*DistMatrix::View(A, 0, m, 0, k0), k0, k1);
            if (k1 < n) {
                P.PermuteRowsRange(*DistMatrix::View(A, 0, m, k1, n), k0, k1);
                auto A11 = DistMatrix::View(A, k0, k1, k0, k1);
                auto A12 = DistMatrix::View(A, k0, k1, k1, n);
                Trsm(ELX_LEFT, ELX_LOWER, ELX_NORMAL, ELX_UNIT, 1.0, *A11, *A12);
                if (k1 < m) {
                    auto A21 = DistMatrix::View(A, k1, m, k0, k1);
                    auto A22 = DistMatrix::View(A, k1, m, k1, n);
                    Gemm(ELX_NORMAL, ELX_NORMAL, -1.0, *A21, *A12, 1.0, *A22, ELX_GEMM_DEFAULT);
                }
            }
        }
        if (gpu) FenceStreams(Ps->Stream(), A.Stream());
    }
    int column = info_host;
    if (gpu && k > 0) {
        ELX_CHECK_HIP(hipMemcpyAsync(&column, info, sizeof(int), hipMemcpyDeviceToHost, A.Stream()));
        ELX_CHECK_HIP(hipStreamSynchronize(A.Stream()));
    }
    if (column != 0) throw SingularMatrixError(column);
    Ap.Finish();
}

namespace lu {
void SolveAfter(int orient, const DistMatrix& A, const Permutation& P, DistMatrix& B) {
    ELX_TRACE("El::lu::SolveAfter");
    ELX_REQUIRE(orient >= ELX_NORMAL && orient <= ELX_ADJOINT, "SolveAfter: bad orientation");
    if (A.Height() != A.Width()) throw LogicError("A must be square");
    if (A.Height() != B.Height()) throw LogicError("A and B must be the same height");
    RequireReal(A.Type(), "LU");
    if (P.Height() != A.Height()) throw LogicError("A and P must be the same height");
    if (orient == ELX_NORMAL) {
        P.PermuteRows(B);
        Trsm(ELX_LEFT, ELX_LOWER, ELX_NORMAL, ELX_UNIT, 1.0, A, B);
        Trsm(ELX_LEFT, ELX_UPPER, ELX_NORMAL, ELX_NON_UNIT, 1.0, A, B);
    } else {
        Trsm(ELX_LEFT, ELX_UPPER, orient, ELX_NON_UNIT, 1.0, A, B);
        Trsm(ELX_LEFT, ELX_LOWER, orient, ELX_UNIT, 1.0, A, B);
        P.InversePermuteRows(B);
    }
}
}  // namespace lu

void LinearSolve(const DistMatrix& A, DistMatrix& B) {
    ELX_TRACE("El::LinearSolve");
    if (A.Height() != A.Width()) throw LogicError("A must be square");
    if (A.Height() != B.Height()) throw LogicError("A and B must be the same height");
    auto F = A.Like(Dist::MC, Dist::MR);
    Copy(A, *F);
    Permutation P;
    LU(*F, P);
    lu::SolveAfter(ELX_NORMAL, *F, P, B);
}

}  // namespace elx
