// El::Gemv, Ger, Symv / Hemv, Syr / Her and Syr2 / Her2 on DistMatrices
// (src/blas_like/level2).  Real types only, so `conjugate` changes nothing:
// Hemv = Symv, Her = Syr, Her2 = Syr2, Geru = Ger.  A vector is an n x 1 or a
// 1 x n DistMatrix of any distribution.
#pragma once
#include "distmatrix.hpp"

namespace elx {

// y := alpha op(A) x + beta y (Gemv.cpp, Gemv/Normal.hpp, Gemv/Transpose.hpp);
// float, double, f16 and bf16
void Gemv(int orient, double alpha, const DistMatrix& A, const DistMatrix& x, double beta, DistMatrix& y);
// beta-less form: y is aligned with A, resized to a column vector and zeroed first
void GemvResize(int orient, double alpha, const DistMatrix& A, const DistMatrix& x, DistMatrix& y);
// The local product on operands that are already spread and aligned with A
// [MC,MR]: NORMAL x [MR,*] or [*,MR], y [MC,*] or [*,MC]; TRANSPOSE the two exchanged
void LocalGemv(int orient, double alpha, const DistMatrix& A, const DistMatrix& x, double beta, DistMatrix& y);
// A += alpha x y^T (Ger.cpp); float and double
void Ger(double alpha, const DistMatrix& x, const DistMatrix& y, DistMatrix& A);
// y := alpha A x + beta y with the symmetric A given by its uplo triangle; the
// other triangle is never read (Symv.cpp); float and double
void Symv(int uplo, double alpha, const DistMatrix& A, const DistMatrix& x, double beta, DistMatrix& y);
namespace symv {
// z[MC,*] += alpha tri(A) x[MR,*],  z[MR,*] += alpha tri'(A)^T x[MC,*], tri the uplo
// triangle with and tri' without the diagonal, on the local block of A [MC,MR]
// (Symv/L.hpp LocalColAccumulateL, Symv/U.hpp); all four vectors aligned with A
void LocalColAccumulate(int uplo, double alpha, const DistMatrix& A, const DistMatrix& x_MC_STAR,
                        const DistMatrix& x_MR_STAR, DistMatrix& z_MC_STAR, DistMatrix& z_MR_STAR);
}  // namespace symv
// A += alpha x x^T on the uplo triangle (Syr.cpp); float and double
void Syr(int uplo, double alpha, const DistMatrix& x, DistMatrix& A);
// A += alpha (x y^T + y x^T) on the uplo triangle (Syr2.cpp); float and double
void Syr2(int uplo, double alpha, const DistMatrix& x, const DistMatrix& y, DistMatrix& A);

}  // namespace elx
