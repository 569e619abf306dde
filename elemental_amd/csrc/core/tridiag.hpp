// El::HermitianTridiag, El::herm_tridiag::ApplyQ and ExplicitCondensed
// (src/lapack_like/condense/HermitianTridiag*).  Real types only, so Hermitian
// and symmetric are the same thing here.
#pragma once
#include "gemm.hpp"

namespace elx {

// Q^T A Q = T in place on the uplo triangle of the n x n column-major A, on the
// buffer itself; the other triangle is neither read nor written.
//   LOWER: for k = 0 .. n-2, H_k = I - tau[k] v v^T, v = [0_{k+1}; 1; A(k+2:n, k)];
//          diag(A) is T's diagonal, A(k+1, k) its subdiagonal.  Q = H_0 .. H_{n-2}
//   UPPER: for k = n-1 .. 1, v = [A(0:k-1, k); 1; 0_{n-k}], scalar tau[k-1];
//          A(k-1, k) is the superdiagonal.  Q = H_{n-1} .. H_1
// The reflector is reflector::Col's (as in LocalQR): beta = -sign(alpha) hypot(alpha,
// |tail|), a tail that is exactly zero (the empty last one included) gives tau = 2
// and beta = -alpha.  tau: n - 1 entries of A's type in A's memory space.
// Device::GPU: blocked in LAPACK's latrd / sytrd form, panels of
// TridiagPanelCols() columns through exec::SytrdPanel, then A22 -= V W^T + W V^T
// on the triangle through TrrkLocal; launches on stream s, no failure mode,
// nothing read back.  Device::CPU: the unblocked column loop.  f64/f32
void LocalHermitianTridiag(Device dev, DType t, int uplo, Int n, void* A, Int ld, void* tau, hipStream_t s);
// the local driver's panel width: kern::kSytrdPanelCols unless SetTridiagPanelCols
// (1 .. kern::kSytrdMaxPanelCols; 0 restores the default) changed it, which only
// the width measurement of tools/tridiag_bench.py does
Int TridiagPanelCols();
void SetTridiagPanelCols(Int w);

// A := the condensed form, t := the n-1 Householder scalars (resized to (n-1) x 1,
// 0 x 1 for n = 0; any distribution).  A 1 x 1 grid runs LocalHermitianTridiag on
// A's buffer.  Any other grid runs the reference's right-looking loop over
// Blocksize() on A [MC,MR] (LowerBlocked.hpp, UpperBlocked.hpp): per panel of nb
// columns each column travels as a [*,*] vector, its reflector and the skinny
// products with the replicated n x nb panels V and W are local exec:: calls, the
// trailing product A22 v is symv::LocalColAccumulate between v[MC,*] and v[MR,*]
// with El::Symv's reduction; then A22 -= V W^T + W V^T as two TrrkLocal calls
// between the panels spread [MC,*] and [MR,*]; the last block of at most nb
// columns is staged [*,*] into the local driver.  LowerPanel.hpp's hand-fused
// messages, the ...Square variants and HermitianTridiagCtrl are not reproduced
void HermitianTridiag(int uplo, DistMatrix& A, DistMatrix& t);

namespace herm_tridiag {
// B := Q B (NORMAL) or Q^T B (TRANSPOSE / ADJOINT) from what HermitianTridiag left
// in A and t (HermitianTridiag/ApplyQ.hpp), blocked by Blocksize().  LEFT only
void ApplyQ(int side, int uplo, int orient, const DistMatrix& A, const DistMatrix& t, DistMatrix& B);
// A := T on the three diagonals of the uplo side, zero elsewhere on that side
// (the reflectors are discarded; the other triangle is left alone)
void ExplicitCondensed(int uplo, DistMatrix& A);
}  // namespace herm_tridiag

}  // namespace elx
