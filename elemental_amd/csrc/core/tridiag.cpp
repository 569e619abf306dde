// El::HermitianTridiag, herm_tridiag::ApplyQ and ExplicitCondensed.
//
// The local GPU driver is LAPACK's sytrd: per panel of w columns the fused panel
// kernels (kernels/sytrd.hip) leave the explicit reflectors V and the vectors W,
// and the trailing triangle gets A22 -= V W^T + W V^T as two TrrkLocal calls (the
// engine Syr2k runs on locally).  Q is a product of n - 1 reflectors stored like
// QR's, so ApplyQ is qr's block-reflector code on the views A(1:n, 0:n-1) and
// B(1:n, :) (LOWER) or A(0:n-1, 1:n) and B(0:n-1, :) (UPPER, unit-upper variant).
#include "tridiag.hpp"
#include "qr.hpp"
#include "level3_internal.hpp"
#include "level2.hpp"
#include "exec.hpp"
#include "../runtime/trace.hpp"
#include <algorithm>
#include <cstdlib>
#include <functional>
#include <memory>
#include <string>

namespace elx {

using namespace detail;

namespace {

void RequireUplo(const char* who, int uplo) {
    ELX_REQUIRE(uplo == ELX_LOWER || uplo == ELX_UPPER, who, ": bad UpperOrLower ", uplo);
}

using DMPtr = std::shared_ptr<DistMatrix>;

void CopyVector(Device dev, DType t, Int len, const char* src, char* dst, hipStream_t s) {
    if (len <= 0) return;
    const kern::Copy2D d{len, 1, src, 1, len, dst, 1, len};
    exec::Copy2DBatch(dev, t, &d, 1, false, 0.0, s);
}

// ELX_TRIDIAG_PANEL=level2: the panel composed from the public Level-2 pieces, the
// baseline the fused kernels are measured against and a second answer for the tests
bool ComposedPanelRequested() {
    const char* e = getenv("ELX_TRIDIAG_PANEL");
    return e && std::string(e) == "level2";
}

// Where a composed panel gets its matrix from: the local buffer, or a distributed
// A through replicated vectors
struct PanelOps {
    // dst[0 .. r1-r0) := A(r0:r1, c), and back
    std::function<void(Int c, Int r0, Int r1, char* dst)> load;
    std::function<void(Int c, Int r0, Int r1, const char* src)> store;
    // y := A(a0:a1, a0:a1) v on the uplo triangle; v and y hold a1 - a0 elements
    std::function<void(Int a0, Int a1, const char* v, char* y)> symv;
};

// What exec::SytrdPanel does, one exec:: call per algebraic step (about twenty
// launches per column), on a replicated copy of the column: the refresh as two
// Gemv, the reflector as a one-column QR leaf (its |beta| multiplied back by the
// signature), v into V, w = t (A22 v - V (W^T v) - W (V^T v)) as ops.symv, four
// Gemv and a scaling by the scalar in device memory (RowScale with stride 0), w -=
// (t/2)(w.v) v as a Gemv, a scaling and a Ger.  UPPER gathers [pivot; tail] into a
// scratch column for the leaf, whose pivot comes first, and scatters it back.  V
// and W are n x w with leading dimension n, indexed by global row.  Either device
void ComposedPanel(Device dev, DType t, bool lower, Int n, Int c0, Int w, const PanelOps& ops, char* tau, char* V,
                   char* W, hipStream_t s) {
    const Int es = (Int)DTypeSize(t);
    Buffer qrwork, g(dev, (size_t)(2 * w + 2) * es, s), vec(dev, (size_t)n * es, s), colbuf(dev, (size_t)n * es, s);
    if (exec::QRWorkBytes(dev, n) > 0) qrwork.Reset(dev, exec::QRWorkBytes(dev, n), s);
    char* g1 = static_cast<char*>(g.data());
    char* g2 = g1 + w * es;
    char* dot = g2 + w * es;
    char* sig = dot + es;
    char* cb = static_cast<char*>(colbuf.data());  // the column, indexed by global row
    auto copy = [&](Int len, const char* src, char* dst) { CopyVector(dev, t, len, src, dst, s); };
    for (Int j = 0; j < w; ++j) {
        const Int c = lower ? c0 + j : c0 - j, rd = c, rp = lower ? c + 1 : c - 1;
        const Int r0 = lower ? c : 0, r1 = lower ? n : c + 1, a0 = lower ? c + 1 : 0, a1 = lower ? n : c, m = a1 - a0;
        char* tj = tau + (lower ? c : c - 1) * es;
        char* vj = V + (a0 + j * n) * es;
        char* wj = W + (a0 + j * n) * es;
        ops.load(c, r0, r1, cb + r0 * es);
        if (j > 0) {
            exec::Gemv(dev, t, false, r1 - r0, j, -1.0, V + r0 * es, n, W + rd * es, n, 1.0, cb + r0 * es, 1, s);
            exec::Gemv(dev, t, false, r1 - r0, j, -1.0, W + r0 * es, n, V + rd * es, n, 1.0, cb + r0 * es, 1, s);
        }
        // the reflector of [pivot; tail]
        char* x = lower ? cb + a0 * es : static_cast<char*>(vec.data());
        if (!lower) {
            copy(1, cb + rp * es, x);
            copy(m - 1, cb, x + es);
        }
        exec::QR(dev, t, m, 1, x, m, tj, sig, qrwork.data(), s);
        exec::RowScale(dev, t, 1, 1, x, 1, sig, 0, 0, s);  // |beta| sig = beta
        if (!lower) {
            copy(1, x, cb + rp * es);
            copy(m - 1, x + es, cb);
        }
        ops.store(c, r0, r1, cb + r0 * es);
        copy(m, cb + a0 * es, vj);
        exec::Fill(dev, t, 1, 1, 1.0, V + (rp + j * n) * es, 1, s);
        exec::Fill(dev, t, 1, 1, 0.0, V + (rd + j * n) * es, 1, s);
        ops.symv(a0, a1, vj, wj);
        if (j > 0) {
            exec::Gemv(dev, t, true, m, j, 1.0, W + a0 * es, n, vj, 1, 0.0, g1, 1, s);
            exec::Gemv(dev, t, true, m, j, 1.0, V + a0 * es, n, vj, 1, 0.0, g2, 1, s);
            exec::Gemv(dev, t, false, m, j, -1.0, V + a0 * es, n, g1, 1, 1.0, wj, 1, s);
            exec::Gemv(dev, t, false, m, j, -1.0, W + a0 * es, n, g2, 1, 1.0, wj, 1, s);
        }
        exec::RowScale(dev, t, m, 1, wj, m, tj, 0, 0, s);
        exec::Gemv(dev, t, true, m, 1, 1.0, wj, m, vj, 1, 0.0, dot, 1, s);
        exec::RowScale(dev, t, 1, 1, dot, 1, tj, 0, 0, s);
        exec::Ger(dev, t, m, 1, -0.5, vj, 1, dot, 1, wj, m, s);
    }
}

// the panel's matrix is the local buffer itself
PanelOps LocalOps(Device dev, DType t, bool lower, char* A, Int ld, hipStream_t s) {
    const Int es = (Int)DTypeSize(t);
    PanelOps ops;
    ops.load = [=](Int c, Int r0, Int r1, char* dst) { CopyVector(dev, t, r1 - r0, A + (r0 + c * ld) * es, dst, s); };
    ops.store = [=](Int c, Int r0, Int r1, const char* src) {
        CopyVector(dev, t, r1 - r0, src, A + (r0 + c * ld) * es, s);
    };
    ops.symv = [=](Int a0, Int a1, const char* v, char* y) {
        exec::SymvAccumulate(dev, t, lower, a1 - a0, a1 - a0, 1.0, A + a0 * (ld + 1) * es, ld, v, 1, v, 1, 0.0, y, 1,
                             nullptr, 1, 0, 1, 0, 1, s);
    };
    return ops;
}

// a [*,*] matrix like A whose local block is a copy of / is copied to a buffer
DMPtr Replicate(const DistMatrix& A, Int h, Int w, const char* src, Int ld) {
    auto R = A.Like(Dist::STAR, Dist::STAR);
    R->Resize(h, w);
    if (h > 0 && w > 0) {
        const kern::Copy2D d{h, w, src, 1, ld, R->Buffer(), 1, std::max<Int>(1, R->LDim())};
        exec::Copy2DBatch(A.Dev(), A.Type(), &d, 1, false, 0.0, R->Stream());
    }
    return R;
}
// src spread over the process rows (MC) or columns (MR) of A22 and aligned with it
DMPtr SpreadLike(const DistMatrix& src, const DistMatrix& A22, Dist d) {
    auto v = A22.Like(d, Dist::STAR);
    v->AlignWith(A22, true);
    Copy(src, *v);
    return v;
}

// the panel's matrix is A [MC,MR]: a column travels as a [*,*] vector, the trailing
// product is symv::LocalColAccumulate between v[MC,*], v[MR,*] and the two partial
// sums, which are added as El::Symv adds them (Symv.cpp:84-91) and replicated
PanelOps DistOps(int uplo, DistMatrix& A) {
    const Int es = (Int)A.ElemSize();
    PanelOps ops;
    ops.load = [&A](Int c, Int r0, Int r1, char* dst) {
        auto R = A.Like(Dist::STAR, Dist::STAR);
        Copy(*DistMatrix::View(A, r0, r1, c, c + 1), *R);
        CopyVector(A.Dev(), A.Type(), r1 - r0, static_cast<const char*>(R->Buffer()), dst, R->Stream());
    };
    ops.store = [&A](Int c, Int r0, Int r1, const char* src) {
        auto R = Replicate(A, r1 - r0, 1, src, r1 - r0);
        auto col = DistMatrix::View(A, r0, r1, c, c + 1);
        Copy(*R, *col);
    };
    ops.symv = [&A, uplo, es](Int a0, Int a1, const char* v, char* y) {
        const Int m = a1 - a0;
        auto A22 = DistMatrix::View(A, a0, a1, a0, a1);
        auto vr = Replicate(A, m, 1, v, m);
        auto x_MC = SpreadLike(*vr, *A22, Dist::MC), x_MR = SpreadLike(*vr, *A22, Dist::MR);
        auto z_MC = A22->Like(Dist::MC, Dist::STAR), z_MR = A22->Like(Dist::MR, Dist::STAR);
        for (auto& z : {z_MC, z_MR}) {
            z->AlignWith(*A22, true);
            z->Resize(m, 1);
            Zero(*z);
        }
        symv::LocalColAccumulate(uplo, 1.0, *A22, *x_MC, *x_MR, *z_MC, *z_MR);
        auto z_MR_MC = A22->Like(Dist::MR, Dist::MC);
        z_MR_MC->Resize(m, 1);
        Zero(*z_MR_MC);
        AxpyContract(1.0, *z_MR, *z_MR_MC);
        auto z = A22->Like(Dist::MC, Dist::MR);
        Copy(*z_MR_MC, *z);
        AxpyContract(1.0, *z_MC, *z);
        auto zr = A.Like(Dist::STAR, Dist::STAR);
        Copy(*z, *zr);
        CopyVector(A.Dev(), A.Type(), m, static_cast<const char*>(zr->Buffer()), y, zr->Stream());
        (void)es;
    };
    return ops;
}

// A22 -= V2 W2^T + W2 V2^T on the uplo triangle of A22 = A(t0:t1, t0:t1) [MC,MR], V
// and W replicated (leading dimension n): the local Trr2k as two TrrkLocal calls
// between the panels spread [MC,*] and [MR,*]
void DistRank2k(bool lower, DistMatrix& A, Int t0, Int t1, Int w, const char* V, const char* W, Int n, Buffer& tmp) {
    const Int es = (Int)A.ElemSize();
    auto A22 = DistMatrix::View(A, t0, t1, t0, t1);
    auto Vr = Replicate(A, t1 - t0, w, V + t0 * es, n), Wr = Replicate(A, t1 - t0, w, W + t0 * es, n);
    auto V_MC = SpreadLike(*Vr, *A22, Dist::MC), V_MR = SpreadLike(*Vr, *A22, Dist::MR);
    auto W_MC = SpreadLike(*Wr, *A22, Dist::MC), W_MR = SpreadLike(*Wr, *A22, Dist::MR);
    auto ld = [](const DMPtr& M) { return std::max<Int>(1, M->LDim()); };
    TrrkLocal(lower, false, true, w, -1.0, V_MC->Buffer(), ld(V_MC), W_MR->Buffer(), ld(W_MR), *A22, A22->Stream(), tmp);
    TrrkLocal(lower, false, true, w, -1.0, W_MC->Buffer(), ld(W_MC), V_MR->Buffer(), ld(V_MR), *A22, A22->Stream(), tmp);
}

}  // namespace

namespace {
Int g_panel_cols = kern::kSytrdPanelCols;
}
Int TridiagPanelCols() { return g_panel_cols; }
void SetTridiagPanelCols(Int w) {
    ELX_REQUIRE(w >= 0 && w <= kern::kSytrdMaxPanelCols, "SetTridiagPanelCols: width ", w, " outside 0 .. ",
                kern::kSytrdMaxPanelCols);
    g_panel_cols = w == 0 ? kern::kSytrdPanelCols : w;
}

void LocalHermitianTridiag(Device dev, DType t, int uplo, Int n, void* A, Int ld, void* tau, hipStream_t s) {
    RequireReal(t, "HermitianTridiag");
    RequireUplo("HermitianTridiag", uplo);
    if (n <= 1) return;
    ELX_REQUIRE(ld >= n && A && tau, "LocalHermitianTridiag: bad arguments");
    const bool lower = uplo == ELX_LOWER;
    const bool composed = ComposedPanelRequested();
    if (dev == Device::CPU && !composed) return exec::HostHermitianTridiag(t, lower, n, A, ld, tau);
    const Int es = (Int)DTypeSize(t), wmax = std::min<Int>(TridiagPanelCols(), n - 1);
    Buffer V(dev, (size_t)n * wmax * es, s), W(dev, (size_t)n * wmax * es, s), work;
    if (!composed) work.Reset(dev, exec::SytrdWorkBytes(n), s);
    Buffer tmp;  // TrrkLocal's masked leaves
    static const auto grid = std::make_shared<Grid>(Comm::Self(), 1, ELX_COLUMN_MAJOR);
    char* a = static_cast<char*>(A);
    // lower: columns 0 .. n-2 upwards; upper: columns n-1 .. 1 downwards
    for (Int done = 0; done < n - 1; done += wmax) {
        const Int w = std::min(wmax, n - 1 - done);
        const Int c0 = lower ? done : n - 1 - done;
        if (composed)
            ComposedPanel(dev, t, lower, n, c0, w, LocalOps(dev, t, lower, a, ld, s), static_cast<char*>(tau),
                          static_cast<char*>(V.data()), static_cast<char*>(W.data()), s);
        else
            exec::SytrdPanel(t, lower, n, c0, w, A, ld, tau, V.data(), W.data(), n, work.data(), s);
        // the trailing block: rows and columns [t0, t1)
        const Int t0 = lower ? c0 + w : 0, t1 = lower ? n : c0 - w + 1;
        DistMatrix A22(grid, t, Dist::MC, Dist::MR, dev);
        A22.Attach(t1 - t0, t1 - t0, 0, 0, a + (t0 + t0 * ld) * es, ld, 0);
        A22.SetStream(s);
        const char* V2 = static_cast<const char*>(V.data()) + t0 * es;
        const char* W2 = static_cast<const char*>(W.data()) + t0 * es;
        TrrkLocal(lower, false, true, w, -1.0, V2, n, W2, n, A22, s, tmp);
        TrrkLocal(lower, false, true, w, -1.0, W2, n, V2, n, A22, s, tmp);
    }
}

void HermitianTridiag(int uplo, DistMatrix& APre, DistMatrix& t) {
    ELX_TRACE("El::HermitianTridiag");
    RequireReal(APre.Type(), "HermitianTridiag");
    RequireUplo("HermitianTridiag", uplo);
    ELX_REQUIRE(&APre.G() == &t.G(), "HermitianTridiag: matrices on different grids");
    ELX_REQUIRE(APre.Type() == t.Type(), "HermitianTridiag: mixed types");
    if (APre.Height() != APre.Width()) throw LogicError("HermitianTridiag: A must be square");
    const Int n = APre.Height();
    auto ts = APre.Like(Dist::STAR, Dist::STAR);
    ts->Resize(std::max<Int>(n - 1, 0), 1);
    const bool local = APre.G().Size() == 1 && APre.Participating() && APre.LocalHeight() == n &&
                       APre.LocalWidth() == n;
    if (n > 1 && local) {
        LocalHermitianTridiag(APre.Dev(), APre.Type(), uplo, n, APre.Buffer(), std::max<Int>(1, APre.LDim()),
                              ts->Buffer(), APre.Stream());
    } else if (n > 1) {
        // the right-looking loop (LowerBlocked.hpp:63-158, UpperBlocked.hpp) over
        // Blocksize(): while more than nb columns are left, a panel of nb columns
        // (ComposedPanel on replicated vectors, its trailing products distributed)
        // and the rank-2 nb update of the trailing triangle; the last block [*,*]
        RWProxy Ap(APre);
        DistMatrix& A = Ap.Get();
        const bool lower = uplo == ELX_LOWER;
        const Device dev = A.Dev();
        const DType ty = A.Type();
        const Int es = (Int)A.ElemSize(), nb = std::max<Int>(1, Blocksize());
        hipStream_t s = A.Stream();
        char* tau = static_cast<char*>(ts->Buffer());
        Buffer V(dev, (size_t)n * nb * es, s), W(dev, (size_t)n * nb * es, s), tmp;
        char* v = static_cast<char*>(V.data());
        char* w = static_cast<char*>(W.data());
        const PanelOps ops = DistOps(uplo, A);
        Int done = 0;
        for (; n - done > nb; done += nb) {
            const Int c0 = lower ? done : n - 1 - done;
            ComposedPanel(dev, ty, lower, n, c0, nb, ops, tau, v, w, s);
            const Int t0 = lower ? done + nb : 0, t1 = lower ? n : n - done - nb;
            DistRank2k(lower, A, t0, t1, nb, v, w, n, tmp);
        }
        const Int m = n - done, b0 = lower ? done : 0;
        if (m > 1) {
            auto last = DistMatrix::View(A, b0, b0 + m, b0, b0 + m);
            auto Ls = A.Like(Dist::STAR, Dist::STAR);
            Copy(*last, *Ls);
            LocalHermitianTridiag(dev, ty, uplo, m, Ls->Buffer(), std::max<Int>(1, Ls->LDim()), tau + b0 * es,
                                  Ls->Stream());
            Copy(*Ls, *last);
        }
        Ap.Finish();
    }
    Copy(*ts, t);
}

namespace herm_tridiag {

void ApplyQ(int side, int uplo, int orient, const DistMatrix& A, const DistMatrix& t, DistMatrix& BPre) {
    ELX_TRACE("El::herm_tridiag::ApplyQ");
    if (side != ELX_LEFT) throw LogicError("ApplyQ: only LEFT is supported");
    RequireUplo("ApplyQ", uplo);
    ELX_REQUIRE(orient >= ELX_NORMAL && orient <= ELX_ADJOINT, "ApplyQ: bad orientation");
    RequireReal(A.Type(), "HermitianTridiag");
    ELX_REQUIRE(&A.G() == &BPre.G() && &A.G() == &t.G(), "ApplyQ: matrices on different grids");
    ELX_REQUIRE(A.Type() == BPre.Type() && A.Type() == t.Type(), "ApplyQ: mixed types");
    if (A.Height() != A.Width()) throw LogicError("ApplyQ: A must be square");
    const Int n = A.Height();
    if (BPre.Height() != n) throw LogicError("ApplyQ: A and B must be the same height");
    if (t.Height() != std::max<Int>(n - 1, 0) || t.Width() != 1) throw LogicError("ApplyQ: t must be (n - 1) x 1");
    if (n <= 1 || BPre.Width() == 0) return;
    MultiSync sync(BPre.Stream(), {A.Stream(), t.Stream()});
    RWProxy Bp(BPre);
    DistMatrix& B = Bp.Get();
    auto tp = ReadProxy(t, B, Dist::STAR, Dist::STAR);
    const bool lower = uplo == ELX_LOWER;
    // the rows Q acts on and the square block that holds its reflectors
    auto P = lower ? DistMatrix::View(A, 1, n, 0, n - 1) : DistMatrix::View(A, 0, n - 1, 1, n);
    auto B1 = lower ? DistMatrix::View(B, 1, n, 0, B.Width()) : DistMatrix::View(B, 0, n - 1, 0, B.Width());
    ApplyPackedReflectors(!lower, orient == ELX_NORMAL, *P, static_cast<const char*>(tp->Buffer()), *B1);
    Bp.Finish();
}

void ExplicitCondensed(int uplo, DistMatrix& A) {
    ELX_TRACE("El::herm_tridiag::ExplicitCondensed");
    RequireUplo("ExplicitCondensed", uplo);
    auto t = A.Like(Dist::STAR, Dist::STAR);
    HermitianTridiag(uplo, A, *t);
    ScaleTrapezoid(0.0, uplo, A, uplo == ELX_LOWER ? -2 : 2);
}

}  // namespace herm_tridiag

}  // namespace elx
