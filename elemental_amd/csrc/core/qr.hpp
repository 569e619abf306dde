// El::QR (Householder), El::qr::ApplyQ / SolveAfter / Explicit / ExplicitTriang
// and El::LeastSquares.
#pragma once
#include "gemm.hpp"

namespace elx {

// A = Q R of the m x n column-major A in place, on the buffer itself: recursion
// over columns down to leaves of kern::kGeqrfLeafCols columns (exec::QR); between
// them the left half's block reflector, transposed, on the right half (GEMM, Trsm
// with the UT transform's triangle, GEMM, in chunks of at most 128 reflectors so
// the triangle stays small), all on stream s.  On return the upper trapezoid holds
// R with a non-negative diagonal, the strict lower part the reflectors, tau and
// sig (k = min(m, n) entries of A's type, in A's memory space) the Householder
// scalars and the signature: Q = H_0 .. H_{k-1} diag(sig).  No failure mode, no
// synchronization, nothing read back.  f64/f32
void LocalQR(Device dev, DType t, Int m, Int n, void* A, Int ld, void* tau, void* sig, hipStream_t s);

// A = Q R in place (src/lapack_like/factor/QR/Householder.hpp): t and d are
// resized to min(m, n) x 1 and receive the Householder scalars and the signature
// (+-1); R has a non-negative diagonal.  f64/f32
void QR(DistMatrix& A, DistMatrix& t, DistMatrix& d);
namespace qr {
// B := Q B (NORMAL) or Q^T B (TRANSPOSE / ADJOINT) from what QR left in A, t and d
// (QR/ApplyQ.hpp with ApplyPacked LLVB / LLVF), blocked by Blocksize().  LEFT only
void ApplyQ(int side, int orient, const DistMatrix& A, const DistMatrix& t, const DistMatrix& d, DistMatrix& B);
// NORMAL: X := argmin ||A X - B||_F = R^-1 (Q^T B)(0:n, :); TRANSPOSE / ADJOINT:
// the minimum-norm X with A^T X = B, Q [R^-T B; 0] (QR/SolveAfter.hpp).  m >= n
void SolveAfter(int orient, const DistMatrix& A, const DistMatrix& t, const DistMatrix& d, const DistMatrix& B,
                DistMatrix& X);
// A := the thin Q (m x k), R := the k x n upper trapezoid (QR/Explicit.hpp)
void Explicit(DistMatrix& A, DistMatrix& R);
// A := R, the k x n upper trapezoid
void ExplicitTriang(DistMatrix& A);
}  // namespace qr
namespace detail {
// B := Q B (normal) or Q^T B for the k = min(height, width) reflectors packed in
// P, B [MC,MR] of P's height, tau replicated in B's memory space, blocked by
// Blocksize() (ApplyPackedReflectors, VERTICAL).  lower: reflector c lies below
// P(c, c), Q = H_0 .. H_{k-1} (LLVF / LLVB, what QR leaves).  upper: it lies above
// P(c, c), Q = H_{k-1} .. H_0 (LUVF / LUVB, what HermitianTridiag(UPPER) leaves
// in A(0:n-1, 1:n)).  No signature.  Shared by qr::ApplyQ and herm_tridiag::ApplyQ
void ApplyPackedReflectors(bool upper, bool normal, const DistMatrix& P, const char* tau, DistMatrix& B);
}  // namespace detail
// X := the least-squares (NORMAL) or minimum-norm (TRANSPOSE / ADJOINT) solution
// for the m x n A, m >= n, factored in a copy (euclidean_min/LeastSquares.cpp);
// m < n (LQ) raises UnsupportedError
void LeastSquares(int orient, const DistMatrix& A, const DistMatrix& B, DistMatrix& X);

}  // namespace elx
