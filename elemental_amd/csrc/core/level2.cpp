// The Level-2 drivers on DistMatrices: the reference's redistributions
// (src/blas_like/level2/Gemv/Normal.hpp, Gemv/Transpose.hpp, Symv.cpp, Ger.cpp,
// Syr.cpp, Syr2.cpp) around one local launch each (exec::Gemv, Ger,
// SymvAccumulate, Syr, Syr2).
#include "level2.hpp"
#include "level3_internal.hpp"
#include "exec.hpp"
#include "../runtime/trace.hpp"

namespace elx {

using namespace detail;

namespace {

bool IsVector(const DistMatrix& v) { return v.Height() == 1 || v.Width() == 1 || v.Height() == 0 || v.Width() == 0; }
Int VecLen(const DistMatrix& v) { return v.Width() == 1 ? v.Height() : v.Height() == 1 ? v.Width() : 0; }
bool IsColumn(const DistMatrix& v) { return v.Width() == 1 || v.Height() != 1; }
// element stride of the local part of a spread vector
Int Inc(const DistMatrix& v) { return IsColumn(v) ? 1 : v.LDim(); }
std::string Dims(const char* name, const DistMatrix& M) { return Cat(name, " ~ ", M.Height(), " x ", M.Width()); }

void RequireUplo(const char* who, int uplo) {
    ELX_REQUIRE(uplo == ELX_LOWER || uplo == ELX_UPPER, who, ": bad UpperOrLower ", uplo);
}
// same grid, type and device for every operand
void RequireTogether(const char* who, const DistMatrix& A, std::initializer_list<const DistMatrix*> others) {
    for (const DistMatrix* o : others) {
        ELX_REQUIRE(&A.G() == &o->G(), who, ": matrices on different grids");
        ELX_REQUIRE(A.Type() == o->Type(), who, ": mixed types (", DTypeName(A.Type()), " and ", DTypeName(o->Type()),
                    ")");
        ELX_REQUIRE(A.Dev() == o->Dev(), who, ": mixed devices");
    }
}

// src spread over A's process columns (d = MR) or rows (d = MC) and aligned with
// A [MC,MR]: [d,*] for a column vector, [*,d] for a row vector, on tgt's stream
DMPtr Spread(const DistMatrix& src, const DistMatrix& A, const DistMatrix& tgt, Dist d) {
    const bool col = IsColumn(src);
    auto v = tgt.Like(col ? d : Dist::STAR, col ? Dist::STAR : d);
    v->AlignWith(A, true);
    Copy(src, *v);
    return v;
}
// a zeroed column vector of length n spread like Spread's
DMPtr ZeroSpread(Int n, const DistMatrix& A, const DistMatrix& tgt, Dist d) {
    auto z = tgt.Like(d, Dist::STAR);
    z->AlignWith(A, true);
    z->Resize(n, 1);
    Zero(*z);
    return z;
}
// y += z for the column vector z; y a column or a row vector
void AddColumn(const DistMatrix& z, DistMatrix& y) {
    if (IsColumn(y)) return Axpy(1.0, z, y);
    auto zt = y.Like(Dist::MC, Dist::MR);
    Transpose(z, *zt);
    Axpy(1.0, *zt, y);
}

void SymvLocal(bool lower, double alpha, const DistMatrix& A, const DistMatrix& x_MC, const DistMatrix& x_MR,
               DistMatrix& z_MC, DistMatrix& z_MR, hipStream_t s) {
    exec::SymvAccumulate(A.Dev(), A.Type(), lower, A.LocalHeight(), A.LocalWidth(), alpha, A.Buffer(), A.LDim(),
                         x_MC.Buffer(), Inc(x_MC), x_MR.Buffer(), Inc(x_MR), 1.0, z_MC.Buffer(), Inc(z_MC),
                         z_MR.Buffer(), Inc(z_MR), A.ColShift(), A.ColStride(), A.RowShift(), A.RowStride(), s);
}

// every rank's local block is the whole matrix, in place
bool WholeLocal(const DistMatrix& M) {
    return M.G().Size() == 1 && M.Participating() && M.LocalHeight() == M.Height() && M.LocalWidth() == M.Width();
}

}  // namespace

void Gemv(int orient, double alpha, const DistMatrix& APre, const DistMatrix& x, double beta, DistMatrix& y) {
    ELX_TRACE("El::Gemv");
    ELX_REQUIRE(orient >= ELX_NORMAL && orient <= ELX_ADJOINT, "Gemv: bad orientation");
    RequireTogether("Gemv", APre, {&x, &y});
    const bool N = orient == ELX_NORMAL;
    const Int ylen = N ? APre.Height() : APre.Width(), xlen = N ? APre.Width() : APre.Height();
    if (!IsVector(x) || !IsVector(y) || VecLen(x) != xlen || VecLen(y) != ylen)
        throw LogicError(Cat("Nonconformal Gemv: ", Dims("A", APre), ", ", Dims("x", x), ", ", Dims("y", y)));
    Scale(beta, y);  // Gemv/Normal.hpp:38 (y *= beta; beta == 0 clears NaNs)
    if (ylen == 0 || xlen == 0 || alpha == 0.0) return;
    MultiSync sync(y.Stream(), {APre.Stream(), x.Stream()});
    auto Ap = ReadProxy(APre, y, Dist::MC, Dist::MR);
    const DistMatrix& A = *Ap;
    // NORMAL: x[MR,*], z[MC,*] := alpha A x[MR,*], y += the sum of z over the
    // process row; TRANSPOSE with MC and MR exchanged
    auto xs = Spread(x, A, y, N ? Dist::MR : Dist::MC);
    auto z = ZeroSpread(ylen, A, y, N ? Dist::MC : Dist::MR);
    exec::Gemv(A.Dev(), A.Type(), !N, A.LocalHeight(), A.LocalWidth(), alpha, A.Buffer(), A.LDim(), xs->Buffer(),
               Inc(*xs), 0.0, z->Buffer(), 1, y.Stream());
    if (IsColumn(y)) return AxpyContract(1.0, *z, y);
    auto zc = y.Like(Dist::MC, Dist::MR);  // Contract, Transpose, Axpy
    zc->Resize(ylen, 1);
    Zero(*zc);
    AxpyContract(1.0, *z, *zc);
    AddColumn(*zc, y);
}

void GemvResize(int orient, double alpha, const DistMatrix& A, const DistMatrix& x, DistMatrix& y) {
    ELX_REQUIRE(orient >= ELX_NORMAL && orient <= ELX_ADJOINT, "Gemv: bad orientation");
    if (!y.Viewing()) y.AlignWith(A, false);
    y.Resize(orient == ELX_NORMAL ? A.Height() : A.Width(), 1);
    Zero(y);
    Gemv(orient, alpha, A, x, 0.0, y);
}

void LocalGemv(int orient, double alpha, const DistMatrix& A, const DistMatrix& x, double beta, DistMatrix& y) {
    ELX_TRACE("El::LocalGemv");
    ELX_REQUIRE(orient >= ELX_NORMAL && orient <= ELX_ADJOINT, "LocalGemv: bad orientation");
    RequireTogether("LocalGemv", A, {&x, &y});
    const bool N = orient == ELX_NORMAL;
    const Int ylen = N ? A.Height() : A.Width(), xlen = N ? A.Width() : A.Height();
    if (!IsVector(x) || !IsVector(y) || VecLen(x) != xlen || VecLen(y) != ylen)
        throw LogicError(Cat("Nonconformal LocalGemv: ", Dims("A", A), ", ", Dims("x", x), ", ", Dims("y", y)));
    // the distribution and alignment of the dimension of A each vector runs along
    const Dist xd = N ? A.RowDist() : A.ColDist(), yd = N ? A.ColDist() : A.RowDist();
    const int xa = N ? A.RowAlign() : A.ColAlign(), ya = N ? A.ColAlign() : A.RowAlign();
    auto fits = [](const DistMatrix& v, Dist d, int align) {
        const bool col = IsColumn(v);
        return (col ? v.ColDist() : v.RowDist()) == d && (col ? v.RowDist() : v.ColDist()) == Dist::STAR &&
               (col ? v.ColAlign() : v.RowAlign()) == align;
    };
    if (!fits(x, xd, xa) || !fits(y, yd, ya))
        throw LogicError("LocalGemv: x and y must be spread over and aligned with the matching dimension of A");
    if (y.LocalHeight() == 0 || y.LocalWidth() == 0) return;
    MultiSync sync(y.Stream(), {A.Stream(), x.Stream()});
    exec::Gemv(A.Dev(), A.Type(), !N, A.LocalHeight(), A.LocalWidth(), alpha, A.Buffer(), A.LDim(), x.Buffer(), Inc(x),
               beta, y.Buffer(), Inc(y), y.Stream());
}

void Ger(double alpha, const DistMatrix& x, const DistMatrix& y, DistMatrix& APre) {
    ELX_TRACE("El::Ger");
    RequireTogether("Ger", APre, {&x, &y});
    RequireReal(APre.Type(), "Ger");
    if (!IsVector(x) || !IsVector(y) || VecLen(x) != APre.Height() || VecLen(y) != APre.Width())
        throw LogicError(Cat("Nonconformal Ger: ", Dims("A", APre), ", ", Dims("x", x), ", ", Dims("y", y)));
    if (APre.Height() == 0 || APre.Width() == 0 || alpha == 0.0) return;
    MultiSync sync(APre.Stream(), {x.Stream(), y.Stream()});
    RWProxy Ap(APre);
    DistMatrix& A = Ap.Get();
    auto xs = Spread(x, A, A, Dist::MC);
    auto ys = Spread(y, A, A, Dist::MR);
    exec::Ger(A.Dev(), A.Type(), A.LocalHeight(), A.LocalWidth(), alpha, xs->Buffer(), Inc(*xs), ys->Buffer(), Inc(*ys),
              A.Buffer(), A.LDim(), A.Stream());
    Ap.Finish();
}

void Symv(int uplo, double alpha, const DistMatrix& APre, const DistMatrix& x, double beta, DistMatrix& y) {
    ELX_TRACE("El::Symv");
    RequireUplo("Symv", uplo);
    RequireTogether("Symv", APre, {&x, &y});
    RequireReal(APre.Type(), "Symv");
    if (APre.Height() != APre.Width()) throw LogicError(Cat("A must be square: ", Dims("A", APre)));
    const Int n = APre.Height();
    if (!IsVector(x) || !IsVector(y) || VecLen(x) != n || VecLen(y) != n)
        throw LogicError(Cat("Nonconformal Symv: ", Dims("A", APre), ", ", Dims("x", x), ", ", Dims("y", y)));
    const bool lower = uplo == ELX_LOWER;
    MultiSync sync(y.Stream(), {APre.Stream(), x.Stream()});
    // one rank, everything already where the kernel wants it: the local Symv
    if (APre.ColDist() == Dist::MC && APre.RowDist() == Dist::MR && WholeLocal(APre) && WholeLocal(x) &&
        WholeLocal(y)) {
        if (n == 0) return;
        exec::SymvAccumulate(y.Dev(), y.Type(), lower, n, n, alpha, APre.Buffer(), APre.LDim(), x.Buffer(), Inc(x),
                             x.Buffer(), Inc(x), beta, y.Buffer(), Inc(y), nullptr, 1, 0, 1, 0, 1, y.Stream());
        return;
    }
    Scale(beta, y);
    if (n == 0 || alpha == 0.0) return;
    auto Ap = ReadProxy(APre, y, Dist::MC, Dist::MR);
    const DistMatrix& A = *Ap;
    auto x_MC = Spread(x, A, y, Dist::MC);
    auto x_MR = Spread(*x_MC, A, y, Dist::MR);
    auto z_MC = ZeroSpread(n, A, y, Dist::MC);
    auto z_MR = ZeroSpread(n, A, y, Dist::MR);
    SymvLocal(lower, alpha, A, *x_MC, *x_MR, *z_MC, *z_MR, y.Stream());
    // Symv.cpp:84-91: z[MR,*] -> [MR,MC] -> [MC,MR], += z[MC,*], y += z
    auto z_MR_MC = y.Like(Dist::MR, Dist::MC);
    z_MR_MC->Resize(n, 1);
    Zero(*z_MR_MC);
    AxpyContract(1.0, *z_MR, *z_MR_MC);
    auto z = y.Like(Dist::MC, Dist::MR);
    Copy(*z_MR_MC, *z);
    AxpyContract(1.0, *z_MC, *z);
    AddColumn(*z, y);
}

void symv::LocalColAccumulate(int uplo, double alpha, const DistMatrix& A, const DistMatrix& x_MC_STAR,
                              const DistMatrix& x_MR_STAR, DistMatrix& z_MC_STAR, DistMatrix& z_MR_STAR) {
    ELX_TRACE("El::symv::LocalColAccumulate");
    RequireUplo("LocalColAccumulate", uplo);
    RequireTogether("LocalColAccumulate", A, {&x_MC_STAR, &x_MR_STAR, &z_MC_STAR, &z_MR_STAR});
    RequireReal(A.Type(), "LocalColAccumulate");
    ELX_REQUIRE(A.ColDist() == Dist::MC && A.RowDist() == Dist::MR, "LocalColAccumulate: A must be [MC,MR]");
    if (A.Height() != A.Width()) throw LogicError(Cat("A must be square: ", Dims("A", A)));
    auto fits = [&](const DistMatrix& v, Dist d, int align) {
        return v.ColDist() == d && v.RowDist() == Dist::STAR && v.ColAlign() == align && v.Height() == A.Height() &&
               v.Width() == 1;
    };
    if (!fits(x_MC_STAR, Dist::MC, A.ColAlign()) || !fits(z_MC_STAR, Dist::MC, A.ColAlign()) ||
        !fits(x_MR_STAR, Dist::MR, A.RowAlign()) || !fits(z_MR_STAR, Dist::MR, A.RowAlign()))
        throw LogicError(Cat("Nonconformal LocalColAccumulate: ", Dims("A", A), ", ", Dims("x[MC,*]", x_MC_STAR), ", ",
                             Dims("x[MR,*]", x_MR_STAR), ", ", Dims("z[MC,*]", z_MC_STAR), ", ",
                             Dims("z[MR,*]", z_MR_STAR), " (or not aligned with A)"));
    if (A.Height() == 0 || alpha == 0.0) return;
    MultiSync sync(z_MC_STAR.Stream(), {A.Stream(), x_MC_STAR.Stream(), x_MR_STAR.Stream(), z_MR_STAR.Stream()});
    SymvLocal(uplo == ELX_LOWER, alpha, A, x_MC_STAR, x_MR_STAR, z_MC_STAR, z_MR_STAR, z_MC_STAR.Stream());
}

void Syr(int uplo, double alpha, const DistMatrix& x, DistMatrix& APre) {
    ELX_TRACE("El::Syr");
    RequireUplo("Syr", uplo);
    RequireTogether("Syr", APre, {&x});
    RequireReal(APre.Type(), "Syr");
    if (APre.Height() != APre.Width()) throw LogicError(Cat("A must be square: ", Dims("A", APre)));
    if (!IsVector(x) || VecLen(x) != APre.Height())
        throw LogicError(Cat("Nonconformal Syr: ", Dims("A", APre), ", ", Dims("x", x)));
    if (APre.Height() == 0 || alpha == 0.0) return;
    MultiSync sync(APre.Stream(), {x.Stream()});
    RWProxy Ap(APre);
    DistMatrix& A = Ap.Get();
    auto x_MC = Spread(x, A, A, Dist::MC);
    auto x_MR = Spread(*x_MC, A, A, Dist::MR);
    exec::Syr(A.Dev(), A.Type(), uplo == ELX_LOWER, A.LocalHeight(), A.LocalWidth(), alpha, x_MC->Buffer(), Inc(*x_MC),
              x_MR->Buffer(), Inc(*x_MR), A.Buffer(), A.LDim(), A.ColShift(), A.ColStride(), A.RowShift(),
              A.RowStride(), A.Stream());
    Ap.Finish();
}

void Syr2(int uplo, double alpha, const DistMatrix& x, const DistMatrix& y, DistMatrix& APre) {
    ELX_TRACE("El::Syr2");
    RequireUplo("Syr2", uplo);
    RequireTogether("Syr2", APre, {&x, &y});
    RequireReal(APre.Type(), "Syr2");
    if (APre.Height() != APre.Width()) throw LogicError(Cat("A must be square: ", Dims("A", APre)));
    if (!IsVector(x) || !IsVector(y) || VecLen(x) != APre.Height() || VecLen(y) != APre.Height())
        throw LogicError(Cat("Nonconformal Syr2: ", Dims("A", APre), ", ", Dims("x", x), ", ", Dims("y", y)));
    if (APre.Height() == 0 || alpha == 0.0) return;
    MultiSync sync(APre.Stream(), {x.Stream(), y.Stream()});
    RWProxy Ap(APre);
    DistMatrix& A = Ap.Get();
    auto x_MC = Spread(x, A, A, Dist::MC);
    auto x_MR = Spread(*x_MC, A, A, Dist::MR);
    auto y_MC = Spread(y, A, A, Dist::MC);
    auto y_MR = Spread(*y_MC, A, A, Dist::MR);
    exec::Syr2(A.Dev(), A.Type(), uplo == ELX_LOWER, A.LocalHeight(), A.LocalWidth(), alpha, x_MC->Buffer(),
               Inc(*x_MC), x_MR->Buffer(), Inc(*x_MR), y_MC->Buffer(), Inc(*y_MC), y_MR->Buffer(), Inc(*y_MR),
               A.Buffer(), A.LDim(), A.ColShift(), A.ColStride(), A.RowShift(), A.RowStride(), A.Stream());
    Ap.Finish();
}

}  // namespace elx
