// El::QR (Householder), qr::ApplyQ / SolveAfter / Explicit / ExplicitTriang and
// LeastSquares.
//
// The block reflector of reflectors u_0 .. u_{nb-1} (U: the explicit m x nb matrix,
// unit diagonal, zero above it) is H_0 .. H_{nb-1} = I - U S^-T U^T with S =
// tril(U^T U), diag(S) = 1 / t (the UT transform; S^-1 + S^-T = U^T U because
// t_j (1 + |u_j|^2) = 2).  So
//   forward  (LLVF.hpp, Q^T B):  Z := U^T B, Z := S^-1 Z, B -= U Z
//   backward (LLVB.hpp, Q B):    Z := U^T B, Z := S^-T Z, B -= U Z
// with Q = H_0 .. H_{k-1} diag(d): NORMAL scales by d first and runs the blocks
// backward, ADJOINT runs them forward and scales last.
#include "qr.hpp"
#include "level3_internal.hpp"
#include "exec.hpp"
#include "../runtime/trace.hpp"
#include <algorithm>

namespace elx {

using namespace detail;

namespace {

// reflectors applied at once by LocalQR: S stays a kApplyBlock-row triangle
constexpr Int kApplyBlock = 128;

// B := H^T B (adjoint) or H B for the block reflector packed in P (m x nb, nb <=
// m), on the local buffers; B is m x n
void LocalApplyBlock(Device dev, DType t, bool adjoint, Int m, Int nb, const char* P, Int ldp, const char* tau, char* B,
                     Int n, Int ldb, hipStream_t s) {
    if (m <= 0 || nb <= 0 || n <= 0) return;
    const size_t es = DTypeSize(t);
    Buffer U(dev, (size_t)m * nb * es, s), S(dev, (size_t)nb * nb * es, s), Z(dev, (size_t)nb * n * es, s);
    exec::QRExplicitU(dev, t, m, nb, P, ldp, U.data(), m, s);
    exec::Gemm(dev, t, true, false, nb, nb, m, 1.0, U.data(), m, U.data(), m, 0.0, S.data(), nb, s);
    exec::QRFixT(dev, t, nb, S.data(), nb, tau, s);
    exec::Gemm(dev, t, true, false, nb, n, m, 1.0, U.data(), m, B, ldb, 0.0, Z.data(), nb, s);
    exec::Trsm(dev, t, true, !adjoint, false, nb, n, S.data(), nb, Z.data(), nb, s);
    exec::Gemm(dev, t, false, false, m, n, nb, -1.0, U.data(), m, Z.data(), nb, 1.0, B, ldb, s);
}

struct LocalQRCall {
    Device dev;
    DType t;
    Int m, ld, es;
    char* A;
    char* tau;
    char* sig;
    void* work;
    hipStream_t s;
    char* at(Int i, Int j) const { return A + (i + j * ld) * es; }
    // Q^T of the reflectors r0..r1-1 on A(r0:m, c0:c1): the blocks forward, then
    // the signature on the top rows
    void ApplyAdjoint(Int r0, Int r1, Int c0, Int c1) const {
        if (c1 <= c0) return;
        for (Int r = r0; r < r1; r += kApplyBlock) {
            const Int nb = std::min(kApplyBlock, r1 - r);
            LocalApplyBlock(dev, t, true, m - r, nb, at(r, r), ld, tau + r * es, at(r, c0), c1 - c0, ld, s);
        }
        exec::RowScale(dev, t, r1 - r0, c1 - c0, at(r0, c0), ld, sig + r0 * es, 0, 1, s);
    }
    // A(c0:m, c0:c1) = Q R by recursion over columns: the left half, its Q^T on
    // the right half, the right half below the split
    void Factor(Int c0, Int c1) const {
        const Int n = c1 - c0;
        if (n <= kern::kGeqrfLeafCols) {
            exec::QR(dev, t, m - c0, n, at(c0, c0), ld, tau + c0 * es, sig + c0 * es, work, s);
            return;
        }
        const Int L = kern::kGeqrfLeafCols, cm = c0 + (n / 2 + L / 2) / L * L;
        Factor(c0, cm);
        ApplyAdjoint(c0, cm, cm, c1);
        Factor(cm, c1);
    }
};

// The packed panel Ps ([*,*], h x nb, nb <= h) as the explicit U and the triangle
// S of its UT transform, both [*,*], computed redundantly on every rank
struct StagedPanel {
    DMPtr U, S;
    // upper: the reflectors lie above the diagonal Ps(off + c, c) (HermitianTridiag(UPPER))
    StagedPanel(const DistMatrix& Ps, const char* tau, bool upper = false, Int off = 0) {
        const Int h = Ps.Height(), nb = Ps.Width();
        U = Ps.Like(Dist::STAR, Dist::STAR);
        U->Resize(h, nb);
        S = Ps.Like(Dist::STAR, Dist::STAR);
        S->Resize(nb, nb);
        const Int ldu = std::max<Int>(1, U->LDim()), lds = std::max<Int>(1, S->LDim());
        hipStream_t s = U->Stream();
        exec::QRExplicitU(Ps.Dev(), Ps.Type(), h, nb, Ps.Buffer(), std::max<Int>(1, Ps.LDim()), U->Buffer(), ldu, s, upper,
                          off);
        exec::Gemm(Ps.Dev(), Ps.Type(), true, false, nb, nb, h, 1.0, U->Buffer(), ldu, U->Buffer(), ldu, 0.0,
                   S->Buffer(), lds, s);
        exec::QRFixT(Ps.Dev(), Ps.Type(), nb, S->Buffer(), lds, tau, s);
    }
    // B := H^T B (adjoint) or H B; B is h x n, [MC,MR]
    void Apply(bool adjoint, DistMatrix& B) const {
        if (B.Width() == 0) return;
        auto Z = B.Like(Dist::MC, Dist::MR);
        Z->Resize(U->Width(), B.Width());
        Gemm(ELX_TRANSPOSE, ELX_NORMAL, 1.0, *U, B, 0.0, *Z, ELX_GEMM_DEFAULT);
        Trsm(ELX_LEFT, ELX_LOWER, adjoint ? ELX_NORMAL : ELX_TRANSPOSE, ELX_NON_UNIT, 1.0, *S, *Z);
        Gemm(ELX_NORMAL, ELX_NORMAL, -1.0, *U, *Z, 1.0, B, ELX_GEMM_DEFAULT);
    }
};

// rows [k0, k1) of B scaled by sig[k0..k1) (sig: replicated, B's type and memory space)
void ScaleRows(DistMatrix& B, Int k0, Int k1, const char* sig) {
    if (k1 <= k0 || B.Width() == 0) return;
    auto V = DistMatrix::View(B, k0, k1, 0, B.Width());
    exec::RowScale(V->Dev(), V->Type(), V->LocalHeight(), V->LocalWidth(), V->Buffer(), std::max<Int>(1, V->LDim()), sig,
                   k0 + V->ColShift(), V->ColStride(), V->Stream());
}

DMPtr Replicated(const DistMatrix& like, Int h, Int w) {
    auto M = like.Like(Dist::STAR, Dist::STAR);
    M->Resize(h, w);
    return M;
}

}  // namespace

void LocalQR(Device dev, DType t, Int m, Int n, void* A, Int ld, void* tau, void* sig, hipStream_t s) {
    RequireReal(t, "QR");
    const Int k = std::min(m, n);
    if (k <= 0) return;
    ELX_REQUIRE(ld >= m && A && tau && sig, "LocalQR: bad arguments");
    Buffer work;  // the leaves' scratch, once per call
    if (exec::QRWorkBytes(dev, m) > 0) work.Reset(dev, exec::QRWorkBytes(dev, m), s);
    const LocalQRCall c{dev, t, m, ld, (Int)DTypeSize(t), static_cast<char*>(A), static_cast<char*>(tau),
                        static_cast<char*>(sig), work.data(), s};
    if (n <= kern::kGeqrfLeafCols) {  // one leaf, m < n included
        exec::QR(dev, t, m, n, A, ld, tau, sig, work.data(), s);
        return;
    }
    c.Factor(0, k);
    c.ApplyAdjoint(0, k, k, n);  // the columns right of the square part only receive Q^T
}

void QR(DistMatrix& APre, DistMatrix& t, DistMatrix& d) {
    ELX_TRACE("El::QR");
    RequireReal(APre.Type(), "QR");
    ELX_REQUIRE(&APre.G() == &t.G() && &APre.G() == &d.G(), "QR: matrices on different grids");
    ELX_REQUIRE(APre.Type() == t.Type() && APre.Type() == d.Type(), "QR: mixed types");
    RWProxy Ap(APre);
    DistMatrix& A = Ap.Get();
    const Int m = A.Height(), n = A.Width(), k = std::min(m, n);
    const Int es = (Int)A.ElemSize();
    // the scalars and the signature as replicated vectors in A's memory space
    auto ts = Replicated(A, k, 1), ds = Replicated(A, k, 1);
    char* tau = static_cast<char*>(ts->Buffer());
    char* sig = static_cast<char*>(ds->Buffer());
    const bool local = SameLocalLayout(A, Dist::STAR, Dist::STAR, 0, 0) && A.LocalHeight() == m && A.LocalWidth() == n;
    if (k > 0 && local) {
        LocalQR(A.Dev(), A.Type(), m, n, A.Buffer(), std::max<Int>(1, A.LDim()), tau, sig, A.Stream());
    } else if (k > 0) {
        // the reference's right-looking loop (QR/Householder.hpp): the panel A(k0:m,
        // k0:k1) factored redundantly on every rank as [*,*], then its Q^T on the
        // columns right of it
        const Int nb = std::max<Int>(1, Blocksize());
        auto Ps = A.Like(Dist::STAR, Dist::STAR);
        for (Int k0 = 0; k0 < k; k0 += nb) {
            const Int k1 = std::min(k, k0 + nb);
            auto panel = DistMatrix::View(A, k0, m, k0, k1);
            Copy(*panel, *Ps);
            LocalQR(A.Dev(), A.Type(), m - k0, k1 - k0, Ps->Buffer(), std::max<Int>(1, Ps->LDim()), tau + k0 * es,
                    sig + k0 * es, Ps->Stream());
            Copy(*Ps, *panel);
            if (k1 < n) {
                auto A2 = DistMatrix::View(A, k0, m, k1, n);
                StagedPanel(*Ps, tau + k0 * es).Apply(true, *A2);
                auto top = DistMatrix::View(A, 0, m, k1, n);
                ScaleRows(*top, k0, k1, sig);
            }
        }
    }
    Copy(*ts, t);
    Copy(*ds, d);
    Ap.Finish();
}

// lower: Q = H_0 .. H_{k-1}, block b is P(k0:m, k0:k1) on B(k0:m, :), NORMAL runs the
// blocks backward with S^-T.  upper: Q = H_{k-1} .. H_0, block b is P(0:k1, k0:k1)
// on B(0:k1, :), and the product in decreasing order makes S^-1 the NORMAL one, the
// blocks forward
void detail::ApplyPackedReflectors(bool upper, bool normal, const DistMatrix& P, const char* tau, DistMatrix& B) {
    const Int m = P.Height(), k = std::min(m, P.Width());
    if (k <= 0 || B.Width() == 0) return;
    const Int es = (Int)P.ElemSize(), nb = std::max<Int>(1, Blocksize()), nB = B.Width();
    auto Ps = B.Like(Dist::STAR, Dist::STAR);
    auto block = [&](Int k0) {
        const Int k1 = std::min(k, k0 + nb);
        const Int i0 = upper ? 0 : k0, i1 = upper ? k1 : m;
        Copy(*DistMatrix::View(P, i0, i1, k0, k1), *Ps);
        auto B1 = DistMatrix::View(B, i0, i1, 0, nB);
        StagedPanel(*Ps, tau + k0 * es, upper, upper ? k0 : 0).Apply(upper ? normal : !normal, *B1);
    };
    if (normal != upper) {
        for (Int k0 = (k - 1) / nb * nb; k0 >= 0; k0 -= nb) block(k0);
    } else {
        for (Int k0 = 0; k0 < k; k0 += nb) block(k0);
    }
}

namespace qr {

void ApplyQ(int side, int orient, const DistMatrix& A, const DistMatrix& t, const DistMatrix& d, DistMatrix& BPre) {
    ELX_TRACE("El::qr::ApplyQ");
    if (side != ELX_LEFT) throw LogicError("ApplyQ: only LEFT is supported");
    ELX_REQUIRE(orient >= ELX_NORMAL && orient <= ELX_ADJOINT, "ApplyQ: bad orientation");
    RequireReal(A.Type(), "QR");
    ELX_REQUIRE(&A.G() == &BPre.G() && &A.G() == &t.G() && &A.G() == &d.G(), "ApplyQ: matrices on different grids");
    ELX_REQUIRE(A.Type() == BPre.Type() && A.Type() == t.Type() && A.Type() == d.Type(), "ApplyQ: mixed types");
    const Int m = A.Height(), k = std::min(m, A.Width());
    if (BPre.Height() != m) throw LogicError("ApplyQ: A and B must be the same height");
    if (t.Height() != k || t.Width() != 1 || d.Height() != k || d.Width() != 1)
        throw LogicError("ApplyQ: t and d must be min(m, n) x 1");
    if (k == 0 || BPre.Width() == 0) return;
    MultiSync sync(BPre.Stream(), {A.Stream(), t.Stream(), d.Stream()});
    RWProxy Bp(BPre);
    DistMatrix& B = Bp.Get();
    auto tp = ReadProxy(t, B, Dist::STAR, Dist::STAR), dp = ReadProxy(d, B, Dist::STAR, Dist::STAR);
    const char* tau = static_cast<const char*>(tp->Buffer());
    const char* sig = static_cast<const char*>(dp->Buffer());
    const bool normal = orient == ELX_NORMAL;
    if (normal) ScaleRows(B, 0, k, sig);
    detail::ApplyPackedReflectors(false, normal, A, tau, B);
    if (!normal) ScaleRows(B, 0, k, sig);
    Bp.Finish();
}

void SolveAfter(int orient, const DistMatrix& A, const DistMatrix& t, const DistMatrix& d, const DistMatrix& B,
                DistMatrix& X) {
    ELX_TRACE("El::qr::SolveAfter");
    ELX_REQUIRE(orient >= ELX_NORMAL && orient <= ELX_ADJOINT, "SolveAfter: bad orientation");
    RequireReal(A.Type(), "QR");
    const Int m = A.Height(), n = A.Width(), nrhs = B.Width();
    if (m < n) throw LogicError("Must have full column rank");
    if (B.Height() != (orient == ELX_NORMAL ? m : n)) throw LogicError("A and B do not conform");
    ELX_REQUIRE(&A.G() == &B.G() && &A.G() == &X.G(), "SolveAfter: matrices on different grids");
    ELX_REQUIRE(A.Type() == B.Type() && A.Type() == X.Type(), "SolveAfter: mixed types");
    auto R = DistMatrix::View(A, 0, n, 0, n);
    auto Y = A.Like(Dist::MC, Dist::MR);
    Y->SetStream(X.Stream());
    if (orient == ELX_NORMAL) {
        Copy(B, *Y);
        ApplyQ(ELX_LEFT, ELX_ADJOINT, A, t, d, *Y);
        auto top = DistMatrix::View(*Y, 0, n, 0, nrhs);
        Trsm(ELX_LEFT, ELX_UPPER, ELX_NORMAL, ELX_NON_UNIT, 1.0, *R, *top);
        Copy(*top, X);
    } else {
        Y->Resize(m, nrhs);
        Zero(*Y);
        auto top = DistMatrix::View(*Y, 0, n, 0, nrhs);
        Copy(B, *top);
        Trsm(ELX_LEFT, ELX_UPPER, ELX_TRANSPOSE, ELX_NON_UNIT, 1.0, *R, *top);
        ApplyQ(ELX_LEFT, ELX_NORMAL, A, t, d, *Y);
        Copy(*Y, X);
    }
}

void ExplicitTriang(DistMatrix& A) {
    ELX_TRACE("El::qr::ExplicitTriang");
    RequireReal(A.Type(), "QR");
    const Int k = std::min(A.Height(), A.Width()), n = A.Width();
    auto t = A.Like(Dist::STAR, Dist::STAR), d = A.Like(Dist::STAR, Dist::STAR);
    QR(A, *t, *d);
    auto R = A.Like(Dist::MC, Dist::MR);
    Copy(*DistMatrix::View(A, 0, k, 0, n), *R);
    ScaleTrapezoid(0.0, ELX_LOWER, *R, -1);
    A.Resize(k, n);
    Copy(*R, A);
}

void Explicit(DistMatrix& A, DistMatrix& R) {
    ELX_TRACE("El::qr::Explicit");
    RequireReal(A.Type(), "QR");
    ELX_REQUIRE(&A.G() == &R.G(), "Explicit: matrices on different grids");
    ELX_REQUIRE(A.Type() == R.Type(), "Explicit: mixed types");
    const Int m = A.Height(), n = A.Width(), k = std::min(m, n);
    auto t = A.Like(Dist::STAR, Dist::STAR), d = A.Like(Dist::STAR, Dist::STAR);
    QR(A, *t, *d);
    auto Rt = A.Like(Dist::MC, Dist::MR);
    Copy(*DistMatrix::View(A, 0, k, 0, n), *Rt);
    ScaleTrapezoid(0.0, ELX_LOWER, *Rt, -1);
    Copy(*Rt, R);
    // Q applied to the first k columns of the identity
    auto Q = A.Like(Dist::MC, Dist::MR);
    Q->Resize(m, k);
    Fill(*Q, 1.0);
    ScaleTrapezoid(0.0, ELX_LOWER, *Q, -1);
    ScaleTrapezoid(0.0, ELX_UPPER, *Q, 1);
    ApplyQ(ELX_LEFT, ELX_NORMAL, A, *t, *d, *Q);
    A.Resize(m, k);
    Copy(*Q, A);
}

}  // namespace qr

void LeastSquares(int orient, const DistMatrix& A, const DistMatrix& B, DistMatrix& X) {
    ELX_TRACE("El::LeastSquares");
    ELX_REQUIRE(orient >= ELX_NORMAL && orient <= ELX_ADJOINT, "LeastSquares: bad orientation");
    RequireReal(A.Type(), "QR");
    if (A.Height() < A.Width()) throw UnsupportedError("LeastSquares: m < n (LQ) is not supported");
    if (B.Height() != (orient == ELX_NORMAL ? A.Height() : A.Width())) throw LogicError("A and B do not conform");
    auto F = A.Like(Dist::MC, Dist::MR);
    Copy(A, *F);
    auto t = A.Like(Dist::STAR, Dist::STAR), d = A.Like(Dist::STAR, Dist::STAR);
    QR(*F, *t, *d);
    qr::SolveAfter(orient, *F, *t, *d, B, X);
}

}  // namespace elx
