// Device-dispatched local primitives.  Device::GPU launches the gfx950 kernels
// (elemental_amd/csrc/kernels); Device::CPU runs the host loops that back the
// reference's Device::CPU DistMatrix path (used when a caller builds CPU
// matrices, e.g. the gloo multi-rank tests).  A GPU matrix never runs here on
// the host: there is no fallback between the two.
#pragma once
#include "../common.hpp"
#include "../runtime/runtime.hpp"
#include "../kernels/kernels.hpp"

namespace elx {
namespace exec {

using kern::Copy2D;

void Copy2DBatch(Device dev, DType t, const Copy2D* d, int nd, bool axpy, double alpha, hipStream_t s);
// dst(i,j) += alpha*src_q(i,j) for every q in order, each rounded to the storage
// type: the rank-ordered sum of AxpyContract in one pass over dst (any number of
// sources: groups of kern::kMaxContractSources, in order)
struct ContractSource { const void* p; Int cs, rs; };
void ContractSum(Device dev, DType t, Int m, Int n, void* dst, Int dcs, Int drs, const ContractSource* src,
                 int nsrc, double alpha, hipStream_t s);
// dst(i,j) = (dst type) src(i,j): Copy_GPU_impl<SrcT,DestT> (Copy.cu:93-205)
void Convert2D(Device dev, DType src_t, DType dst_t, const Copy2D& d, hipStream_t s);
// C := alpha op(A) op(B) + beta C.  Large f64 / f32 products take one or two levels
// of Strassen-Winograd over GemmPlain (strassen.hpp says which); GemmLastLevels: how
// many levels the last Gemm of this thread used (0: the plain kernel)
void Gemm(Device dev, DType t, bool ta, bool tb, Int m, Int n, Int k, double alpha,
          const void* A, Int lda, const void* B, Int ldb, double beta, void* C, Int ldc, hipStream_t s);
// the plain kernel (host: cpu_gemm), whatever the shape
void GemmPlain(Device dev, DType t, bool ta, bool tb, Int m, Int n, Int k, double alpha,
               const void* A, Int lda, const void* B, Int ldb, double beta, void* C, Int ldc, hipStream_t s);
int GemmLastLevels();
// the additions of a Strassen-Winograd level (kernels.hpp): D := X + sy Y for nq
// <= 2 descriptors, and C_t := beta_t C_t + coef_t M for up to two targets; f64/f32
void QuadSum(Device dev, DType t, const kern::QuadSum* q, int nq, hipStream_t s);
void QuadScatter(Device dev, DType t, const kern::QuadScatter& q, hipStream_t s);
void Fill(Device dev, DType t, Int m, Int n, double v, void* A, Int lda, hipStream_t s);
void Scale(Device dev, DType t, Int m, Int n, double alpha, void* A, Int lda, hipStream_t s);
// Frobenius-norm pieces: max |a| (NaN propagates) and sum (a / scale)^2, in double
double AbsMax(Device dev, DType t, Int m, Int n, const void* A, Int lda, hipStream_t s);
double ScaledSumSq(Device dev, DType t, Int m, Int n, const void* A, Int lda, double scale, hipStream_t s);
void Hadamard(Device dev, DType t, Int m, Int n, const void* A, Int lda, const void* B, Int ldb,
              void* C, Int ldc, hipStream_t s);
void Map(Device dev, DType t, int fn, Int m, Int n, const void* A, Int lda, void* B, Int ldb, hipStream_t s);
void Combine(Device dev, DType t, int fn, Int m, Int n, const void* A, Int lda, void* B, Int ldb, hipStream_t s);
// Y := beta*Y + alpha*X (X null: beta*Y) on the lower/upper trapezoid of the
// global index map (i0 + i*is, j0 + j*js) (ScaleTrapezoid.hpp, AxpyTrapezoid)
void Trapezoid(Device dev, DType t, bool lower, Int m, Int n, double alpha, const void* X, Int ldx, double beta,
               void* Y, Int ldy, Int i0, Int is, Int j0, Int js, Int offset, hipStream_t s);
// op(A) X = B in place, A m x m (LocalTrsm / blas::Trsm, Left side); f64/f32
void Trsm(Device dev, DType t, bool lower, bool trans, bool unit, Int m, Int n, const void* A, Int lda, void* B,
          Int ldb, hipStream_t s);
// B := alpha * op(tri(A)) * B in place (LocalTrmm / blas::Trmm, Left side); f64/f32
void Trmm(Device dev, DType t, bool lower, bool trans, bool unit, Int m, Int n, double alpha, const void* A, Int lda,
          void* B, Int ldb, hipStream_t s);
// A = L L^T (lower) / U^T U in place on the uplo triangle of the n x n A, n <=
// kern::kPotrfMax on the GPU (LowerVariant3Unblocked, LowerVariant3.hpp:17-50).
// A pivot that is not > 0 stops it and stores col0 + j + 1 in *info if that is
// still 0; a non-zero *info on entry makes the call a no-op.  info is device
// memory for Device::GPU, host memory for Device::CPU.  f64/f32
void Cholesky(Device dev, DType t, bool lower, Int n, void* A, Int lda, int* info, int col0, hipStream_t s);
// P A = L U of the m x w column panel A in place, w <= kern::kGetrfLeafCols <= m
// (lu::Panel, LU/Panel.hpp): piv[j] = row_off + the row that was swapped with row
// j at step j.  The largest |value| pivots, ties to the smallest row, a NaN never
// beats a number.  An exactly zero pivot (or nothing but zeros and NaNs left)
// stops it and stores col0 + j + 1 in *info if that is still 0; a non-zero
// *info on entry makes the call a no-op.  piv, info and work (LUWorkBytes(dev,
// m) bytes, the GPU kernels' scratch) live in the matrix's memory space.  On
// the GPU this is launches and nothing else.  f64/f32
size_t LUWorkBytes(Device dev, Int m);
void LU(Device dev, DType t, Int m, Int w, void* A, Int lda, int* piv, int row_off, void* work, int* info, int col0,
        hipStream_t s);
// rows k and piv[k] - voff of the m x n A swapped for k = k0..k1-1 (inverse: in
// the opposite order); bit-exact.  info (may be null): non-zero makes it a no-op
void Laswp(Device dev, DType t, Int m, Int n, void* A, Int lda, const int* piv, Int k0, Int k1, Int voff, bool inverse,
           const int* info, hipStream_t s);
// A = Q R of the m x w column panel A in place, w <= kern::kGeqrfLeafCols, any m
// (qr::PanelHouseholder with reflector::Col): R with a non-negative diagonal in
// the upper trapezoid, the reflectors u_j (implicit leading 1) below it, tau[j]
// the Householder scalars and sig[j] = +-1 the signature, k = min(m, w) of each
// in the matrix's type; Q = H_0 .. H_{k-1} diag(sig), H_j = I - tau_j [1; u_j]
// [1; u_j]^T.  A column that is zero below the diagonal gets tau = 2.  Norms and
// dots are scaled by the column's largest magnitude, so no stored range
// overflows; the reference's rescue loop for subnormal columns is left out.  NaN
// and Inf propagate.  tau, sig and work (QRWorkBytes(dev, m) bytes) live in the
// matrix's memory space.  On the GPU this is launches and nothing else.  f64/f32
size_t QRWorkBytes(Device dev, Int m);
void QR(Device dev, DType t, Int m, Int w, void* A, Int lda, void* tau, void* sig, void* work, hipStream_t s);
// U (m x nb) := the reflectors packed below A's diagonal, made explicit (zero
// above the diagonal, 1 on it).  upper: the reflectors packed above the diagonal
// A(off + c, c) instead (zero below it, 1 on it), as HermitianTridiag(UPPER) leaves them
void QRExplicitU(Device dev, DType t, Int m, Int nb, const void* A, Int lda, void* U, Int ldu, hipStream_t s,
                 bool upper = false, Int off = 0);
// Device::GPU: one panel of the blocked tridiagonalization (kern::sytrd_panel):
// columns c0, c0 +- 1, .. (w of them, at most kern::kSytrdMaxPanelCols) of the n x n
// A's uplo triangle are reduced; V and W (n x w, leading dimension ldv) receive the
// explicit reflectors and the vectors of the update owed to the trailing triangle,
// A22 -= V W^T + W V^T.  work: SytrdWorkBytes(n) bytes.  Launches and nothing else
size_t SytrdWorkBytes(Int n);
void SytrdPanel(DType t, bool lower, Int n, Int c0, Int w, void* A, Int lda, void* tau, void* V, void* W, Int ldv,
                void* work, hipStream_t s);
// Device::CPU: the whole reduction Q^T A Q = T as the unblocked column loop
// (herm_tridiag::LowerBlocked / UpperBlocked's sequential form), same conventions
void HostHermitianTridiag(DType t, bool lower, Int n, void* A, Int lda, void* tau);
// S (nb x nb) := tril(S) with diag(S) = 1 / tau (FixDiagonal, ApplyPacked/LLVF.hpp)
void QRFixT(Device dev, DType t, Int nb, void* S, Int lds, const void* tau, hipStream_t s);
// A(i, :) *= sig[i0 + i * is] (DiagonalScale(LEFT) by a vector of A's type and memory space)
void RowScale(Device dev, DType t, Int m, Int n, void* A, Int lda, const void* sig, Int i0, Int is, hipStream_t s);
// A := tri(A)^-1 in place on the uplo triangle of the n x n A (unit: the
// diagonal is neither read nor written), n <= kern::kTrtriMax on the GPU
// (triang_inv::LVar3Unb / UVar3Unb).  No singularity test.  f64/f32
void TriangularInverse(Device dev, DType t, bool lower, bool unit, Int n, void* A, Int lda, hipStream_t s);
// A := L^T L (lower) / U U^T (upper) in place on the uplo triangle, n <=
// kern::kTrtriMax on the GPU (trtrmm::LUnblocked / UUnblocked).  f64/f32
void Trtrmm(Device dev, DType t, bool lower, Int n, void* A, Int lda, hipStream_t s);
// GPU only: W_b := op(A_bb)^-1 for every nb x nb diagonal block of the m x m A
// (W_b at W + b*nb*nb, leading dimension nb), one launch
void TriInverseBatched(DType t, bool lower, bool trans, bool unit, Int nb, Int m, const void* A, Int lda, void* W,
                       hipStream_t s);
// B := W B (W m x m) through a workspace: one MFMA GEMM + one copy
void ApplyInverse(Device dev, DType t, Int m, Int n, const void* W, Int ldw, void* B, Int ldb, hipStream_t s);
void FillHash(Device dev, DType t, Int m, Int n, void* A, Int lda, Int i0, Int is, Int j0, Int js,
              uint64_t seed, double center, double radius, hipStream_t s);
// ---- Level 2 (kernels/level2.hip on the GPU).  Vectors have an element stride
// >= 1; sums are kept in double (f64) or float (the other types) and rounded once.
// y := alpha op(A) x + beta y, A m x n (blas::Gemv).  beta == 0: y is not read;
// alpha == 0 or a zero-length x: y := beta y without reading A or x.  All four types
void Gemv(Device dev, DType t, bool trans, Int m, Int n, double alpha, const void* A, Int lda, const void* x, Int incx,
          double beta, void* y, Int incy, hipStream_t s);
// A += alpha x y^T, A m x n (blas::Geru).  f64/f32
void Ger(Device dev, DType t, Int m, Int n, double alpha, const void* x, Int incx, const void* y, Int incy, void* A,
         Int lda, hipStream_t s);
// symv::LocalColAccumulateL / U on the m x n block whose element (i, j) is global
// (i0 + i is, j0 + j js), without the reference's copies of the diagonal blocks:
//   zr[i] := beta zr[i] + alpha sum_{j: gj <= gi} a(i,j) xc[j]     (lower; upper
//   zc[j] := beta zc[j] + alpha sum_{i: gi >  gj} a(i,j) xr[i]      mirrored)
// xr, zr are indexed by local row, xc, zc by local column; an element on the
// other side of the diagonal is never read.  zc null (m == n): both sums go to
// zr, which with the identity map is blas::Symv.  f64/f32
void SymvAccumulate(Device dev, DType t, bool lower, Int m, Int n, double alpha, const void* A, Int lda,
                    const void* xr, Int incxr, const void* xc, Int incxc, double beta, void* zr, Int inczr, void* zc,
                    Int inczc, Int i0, Int is, Int j0, Int js, hipStream_t s);
// A(i,j) += alpha xr[i] xc[j] on the lower / upper triangle of the same index
// map; the other triangle is neither read nor written (blas::Syr).  f64/f32
void Syr(Device dev, DType t, bool lower, Int m, Int n, double alpha, const void* xr, Int incxr, const void* xc,
         Int incxc, void* A, Int lda, Int i0, Int is, Int j0, Int js, hipStream_t s);
// A(i,j) += alpha (xr[i] yc[j] + yr[i] xc[j]) likewise (blas::Syr2).  f64/f32
void Syr2(Device dev, DType t, bool lower, Int m, Int n, double alpha, const void* xr, Int incxr, const void* xc,
          Int incxc, const void* yr, Int incyr, const void* yc, Int incyc, void* A, Int lda, Int i0, Int is, Int j0,
          Int js, hipStream_t s);
// host-side scalar conversion of one element (for Get/Set and tests)
double LoadScalar(DType t, const void* p);
void StoreScalar(DType t, void* p, double v);

}  // namespace exec
}  // namespace elx
