// El::LU with partial pivoting, El::lu::SolveAfter and El::LinearSolve.
#pragma once
#include "gemm.hpp"
#include "permutation.hpp"

namespace elx {

// P A = L U of the m x n column-major A in place (L unit lower, U upper, min(m, n)
// pivots), on the buffer itself: Toledo's recursion over columns down to leaves of
// kern::kGetrfLeafCols columns (exec::LU), with exec::Laswp, a unit-lower solve
// (exec::Trsm on the CPU; on the GPU 64-row blocks of the substitution kernel
// joined by GEMMs, see lu.cpp) and exec::Gemm between them, all on stream s.  piv[j] = col0 + the row that was swapped with
// row j; piv and info live in A's memory space.  An exactly zero pivot stores
// col0 + column + 1 in *info if that is still 0 and the rest of the call does
// nothing of consequence (A is then unspecified); nothing is read back.  f64/f32
void LocalLU(Device dev, DType t, Int m, Int n, void* A, Int ld, int* piv, int* info, int col0, hipStream_t s);

// P A = L U in place with partial pivoting (src/lapack_like/factor/LU.cpp:88-131);
// P is reset to A's height, device and stream and receives the min(m, n) swaps.
// SingularMatrixError (on every rank, naming the 1-based column) when a pivot is
// exactly zero; A and P are then unspecified.  f64/f32
void LU(DistMatrix& A, Permutation& P);
namespace lu {
// B := op(A)^-1 B from the factors LU left in A and P (LU/SolveAfter.hpp:94-121)
void SolveAfter(int orient, const DistMatrix& A, const Permutation& P, DistMatrix& B);
}  // namespace lu
// B := A^-1 B; A is factored in a copy (src/lapack_like/solve/Linear.cpp)
void LinearSolve(const DistMatrix& A, DistMatrix& B);

}  // namespace elx
