/*
 * elemental_amd.h — C-ABI boundary of the MI355X-native El::Gemm path.
 *
 * Every entry point is `extern "C"`, takes plain pointers / sizes / enums,
 * never throws, returns 0 on success and a nonzero ELX_ERR_* code on failure
 * (message via elx_last_error()).  Device work is stream-ordered on the
 * hipStream_t passed as `void* stream` (NULL = the library's compute stream).
 * Callers keep ownership of every buffer they pass in.
 *
 * Each group below names the reference interface it replaces
 * (paths relative to the reference tree, aj-prime/Elemental = LLNL Hydrogen).
 */
#ifndef ELEMENTAL_AMD_H
#define ELEMENTAL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (mapped back to the reference's exception types) ------ */
#define ELX_OK                  0
#define ELX_ERR_LOGIC           1  /* El::LogicError  (std::logic_error)        */
#define ELX_ERR_HIP             2  /* hydrogen::HIPError (H_CHECK_HIP)           */
#define ELX_ERR_COMM            3  /* El::mpi error / Aluminum error             */
#define ELX_ERR_RUNTIME         4  /* El::RuntimeError                           */
#define ELX_ERR_UNSUPPORTED     5  /* "Bad device/type combo" LogicErrors        */
#define ELX_ERR_NO_DEVICE       6  /* no gfx950 device visible                   */
#define ELX_ERR_SINGULAR        7  /* El::SingularMatrixException                */
#define ELX_ERR_NOT_HPD         8  /* El::NonHPDMatrixException (elx_last_nonhpd_column) */

/* ---- enums: ordinals match the reference ------------------------------- */
/* El::Orientation  include/El/core/types.hpp:463-469 */
#define ELX_NORMAL     0
#define ELX_TRANSPOSE  1
#define ELX_ADJOINT    2
/* El::Dist  include/El/core/types.hpp:207-217 */
#define ELX_MC    0
#define ELX_MD    1
#define ELX_MR    2
#define ELX_VC    3
#define ELX_VR    4
#define ELX_STAR  5
#define ELX_CIRC  6
/* El::GemmAlgorithm  include/El/blas_like/level3.hpp:22-35 */
#define ELX_GEMM_DEFAULT    0
#define ELX_GEMM_SUMMA_A_MS 1
#define ELX_GEMM_SUMMA_A    2
#define ELX_GEMM_SUMMA_B_MS 3
#define ELX_GEMM_SUMMA_B    4
#define ELX_GEMM_SUMMA_C_MS 5
#define ELX_GEMM_SUMMA_C    6
#define ELX_GEMM_SUMMA_DOT  7
#define ELX_GEMM_CANNON     8
/* El::UpperOrLower  include/El/core/types.hpp:511-515 */
#define ELX_LOWER 0
#define ELX_UPPER 1
/* El::LeftOrRight / El::UnitOrNonUnit  include/El/core/types.hpp:418-422,489-493 */
#define ELX_LEFT     0
#define ELX_RIGHT    1
#define ELX_NON_UNIT 0
#define ELX_UNIT     1
/* El::GridOrder  include/El/core/types.hpp:408-413 */
#define ELX_ROW_MAJOR    0
#define ELX_COLUMN_MAJOR 1
/* El::Device  include/hydrogen/Device.hpp */
#define ELX_DEVICE_CPU 0
#define ELX_DEVICE_GPU 1
/* element types (the reference's GPU compute types + bf16, which it lacks) */
#define ELX_F32  0
#define ELX_F64  1
#define ELX_F16  2   /* gpu_half_type (rocblas_half), include/hydrogen/utils/HalfPrecision.hpp:123 */
#define ELX_BF16 3   /* new: no reference counterpart */
/* element types of the communication entry points only (elx_mpi_*, elx_comm_*):
 * El::mpi's collectives also move Int / int / byte buffers (El::Int is 64-bit
 * in an EL_USE_64BIT_INTS build, 32-bit by default) */
#define ELX_I32  4
#define ELX_I64  5
#define ELX_U8   6
/* entrywise functors for elx_entrywise_map (the C-ABI cannot carry a device
 * lambda; include/El.hpp maps them to El::EntrywiseFn)      */
#define ELX_MAP_IDENTITY 0
#define ELX_MAP_NEGATE   1
#define ELX_MAP_ABS      2
#define ELX_MAP_SQUARE   3
#define ELX_MAP_SQRT     4
#define ELX_MAP_EXP      5
#define ELX_MAP_LOG      6
#define ELX_MAP_RELU     7
#define ELX_MAP_SIGMOID  8
#define ELX_MAP_RECIP    9
#define ELX_MAP_TANH     10
/* binary functors for elx_combine: B(i,j) := f(A(i,j), B(i,j))
 * (El::Combine, include/El/blas_like/level1/EntrywiseMap.hpp:170-202) */
#define ELX_COMBINE_ADD       0   /* a + b                 */
#define ELX_COMBINE_SUB       1   /* b - a                 */
#define ELX_COMBINE_MUL       2   /* a * b                 */
#define ELX_COMBINE_DIV       3   /* b / a                 */
#define ELX_COMBINE_MAX       4   /* max(a, b)             */
#define ELX_COMBINE_MIN       5   /* min(a, b)             */
#define ELX_COMBINE_RELU_GRAD 6   /* a > 0 ? b : 0         */

/* ---- errors / runtime --------------------------------------------------- */
/* replaces hydrogen::HIPError / H_CHECK_HIP (include/hydrogen/device/gpu/rocm/ROCmError.hpp) */
const char* elx_last_error(void);
/* after ELX_ERR_NOT_HPD on this thread: the 1-based column of the first pivot that was not > 0 */
int elx_last_nonhpd_column(void);
int elx_version(void);
/* replaces hydrogen::gpu::Initialize / ComputeDeviceId (src/hydrogen/device/GPU.cpp:30-67) */
int elx_device_count(int* count);
int elx_set_device(int device);
int elx_get_device(int* device);
int elx_device_synchronize(void);
/* replaces SyncInfo<Device::GPU> {stream, event} (include/hydrogen/device/gpu/rocm/SyncInfo.hpp:15-41) */
int elx_default_stream(void** stream);
/* the high-priority stream the SUMMA drivers move panels on */
int elx_comm_stream(void** stream);
/* CUs masked off the compute stream for communication kernels (env ELX_COMM_CUS,
 * read at device initialisation; 0 = none) */
int elx_reserved_cus(int* cus);
int elx_stream_create(void** stream);
int elx_stream_destroy(void* stream);
int elx_stream_synchronize(void* stream);
/* the event half of SyncInfo<Device::GPU> and the fences built on it
 * (include/hydrogen/device/gpu/rocm/SyncInfo.hpp:15-81: AddSynchronizationPoint
 * = record, AddSyncPoint = stream waits on event; ROCm.cpp:58-66 default event).
 * Events are created with timing disabled, as the reference's. */
int elx_default_event(void** event);
int elx_event_create(void** event);
int elx_event_destroy(void* event);
int elx_event_record(void* event, void* stream);
int elx_stream_wait_event(void* stream, void* event);
int elx_event_synchronize(void* event);

/* ---- device memory pool: replaces the hipCUB CachingDeviceAllocator -----
 * (src/core/imports/cub.cpp:1-75, El::Memory mode 1 include/El/core/Memory/impl.hpp:113-187) */
int elx_pool_alloc(void** ptr, size_t bytes, void* stream);
int elx_pool_free(void* ptr, void* stream);
int elx_pool_trim(size_t bytes_to_keep);
int elx_pool_stats(size_t* bytes_reserved, size_t* bytes_in_use);
/* cap on the bytes held in the cache (H_CUB_MAX_CACHED_SIZE, cub.cpp:37-43;
 * SIZE_MAX = unbounded, the default); lowering it releases cached blocks */
int elx_pool_set_max_cached(size_t bytes);
int elx_pool_max_cached(size_t* bytes);
/* the bin a request of `bytes` is served from (reserved bytes per block);
 * H_CUB_BIN_GROWTH / H_CUB_MIN_BIN / H_CUB_MAX_BIN select CUB's geometric bins
 * (cub.cpp:21-35, read once per process); 0 when no bin can hold the request
 * (its rounding overflows size_t: elx_pool_alloc fails with out-of-memory) */
size_t elx_pool_bin_bytes(size_t bytes);
/* 1 when a request of `bytes` is cached on free, 0 when it is above
 * H_CUB_MAX_BIN's bin (an own-size block returned to the driver on free) */
int elx_pool_bin_cacheable(size_t bytes);
/* bytes the allocator holds from the driver (hipMalloc'd, not yet hipFree'd):
 * its live and cached blocks */
int elx_pool_backing_reserved(size_t* bytes);
int elx_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int elx_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int elx_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);

/* ---- local GEMM: replaces hydrogen::gpu_blas::Gemm -> rocblas_{h,s,d}gemm
 * (include/hydrogen/blas/GPU_BLAS_impl.hpp:397-423, src/hydrogen/device/rocBLAS_API.cpp:151-170).
 * Column-major C(m x n) := alpha op(A) op(B) + beta C; beta == 0 never reads C.
 * f16/bf16 take/return 16-bit storage, accumulate in f32. */
int elx_gemm_f64(int opA, int opB, int64_t m, int64_t n, int64_t k,
                 double alpha, const double* A, int64_t lda,
                 const double* B, int64_t ldb,
                 double beta, double* C, int64_t ldc, void* stream);
int elx_gemm_f32(int opA, int opB, int64_t m, int64_t n, int64_t k,
                 float alpha, const float* A, int64_t lda,
                 const float* B, int64_t ldb,
                 float beta, float* C, int64_t ldc, void* stream);
/* How many Strassen-Winograd levels the last local GEMM of the calling thread used
 * (0: the plain kernel).  Large f64 / f32 products take one level by default, and
 * two where the half-size products are themselves large enough.  ELX_GEMM_STRASSEN
 * (0 off, 1, 2 levels), ELX_GEMM_STRASSEN_MIN (the threshold on min(m, n, k)) and
 * ELX_GEMM_STRASSEN_MIN2 (the threshold on a half-size product's min(m, n, k) for
 * the second level) are read at every call.  For tests. */
int elx_gemm_last_levels(void);
int elx_gemm_f16(int opA, int opB, int64_t m, int64_t n, int64_t k,
                 float alpha, const uint16_t* A, int64_t lda,
                 const uint16_t* B, int64_t ldb,
                 float beta, uint16_t* C, int64_t ldc, void* stream);
int elx_gemm_bf16(int opA, int opB, int64_t m, int64_t n, int64_t k,
                  float alpha, const uint16_t* A, int64_t lda,
                  const uint16_t* B, int64_t ldb,
                  float beta, uint16_t* C, int64_t ldc, void* stream);

/* ---- El::Matrix<T,D> on either device (device = ELX_DEVICE_*; stream ignored on
 * the CPU).  gemm replaces Gemm(Orientation, Orientation, T, Matrix<T,D> const&,
 * Matrix<T,D> const&, T, Matrix<T,D>&) (include/El/blas_like/level3.hpp:37-65,
 * src/blas_like/level3/Gemm.cpp:141-250; k == 0 -> C := beta C); fill / scale /
 * axpy / copy replace El::Fill / Scale / Axpy / Copy on Matrix<T,D>
 * (include/El/blas_like/level1/{Fill,Scale,Axpy,Copy}.hpp). */
int elx_matrix_gemm(int dtype, int device, int opA, int opB, int64_t m, int64_t n, int64_t k,
                    double alpha, const void* A, int64_t lda, const void* B, int64_t ldb,
                    double beta, void* C, int64_t ldc, void* stream);
int elx_matrix_fill(int dtype, int device, int64_t m, int64_t n, double value,
                    void* A, int64_t lda, void* stream);
int elx_matrix_scale(int dtype, int device, int64_t m, int64_t n, double alpha,
                     void* A, int64_t lda, void* stream);
int elx_matrix_axpy(int dtype, int device, int64_t m, int64_t n, double alpha,
                    const void* X, int64_t ldx, void* Y, int64_t ldy, void* stream);
int elx_matrix_copy(int dtype, int device, int64_t m, int64_t n, const void* A, int64_t lda,
                    void* B, int64_t ldb, void* stream);
/* El::Trmm on Matrix<T> (src/blas_like/level3/Trmm.cpp:23-51): B (m x n) := alpha
 * op(tri(A)) B (LEFT, A m x m) or alpha B op(tri(A)) (RIGHT, A n x n), in place;
 * only A's uplo triangle is read (and no diagonal when UNIT).  f32/f64. */
int elx_matrix_trmm(int dtype, int device, int side, int uplo, int orient, int diag,
                    int64_t m, int64_t n, double alpha, const void* A, int64_t lda,
                    void* B, int64_t ldb, void* stream);
/* El::Trsm on Matrix<T> (src/blas_like/level3/Trsm.cpp:80-127): B (m x n) := alpha
 * op(tri(A))^-1 B (LEFT, A m x m) or alpha B op(tri(A))^-1 (RIGHT, A n x n), in place;
 * only A's uplo triangle is read (and no diagonal when UNIT).  f32/f64. */
int elx_matrix_trsm(int dtype, int device, int side, int uplo, int orient, int diag,
                    int64_t m, int64_t n, double alpha, const void* A, int64_t lda,
                    void* B, int64_t ldb, void* stream);
/* The GPU path of a LEFT solve with an m x m triangle and n right-hand sides:
 * *invert (the block is inverted and applied as one GEMM, else substitution),
 * *lds (the kernel keeps the right-hand sides in LDS, else in global memory) and
 * the LDS bytes of that launch.  elx_trsm_last_launch: what the last local solve of
 * this process launched, 1 (inverse) | 2 (LDS kernel), -1 before any.  For tests. */
int elx_trsm_plan(int dtype, int64_t m, int64_t n, int* invert, int* lds, int64_t* lds_bytes);
int elx_trsm_last_launch(void);
/* El::Cholesky on Matrix<T> (src/lapack_like/factor/Cholesky.cpp): the n x n A :=
 * its Cholesky factor, in place on the uplo triangle (A = L L^T for ELX_LOWER, U^T U
 * for ELX_UPPER); the other triangle is neither read nor written.  Runs the blocked
 * driver of elx_cholesky on the buffer.  ELX_ERR_NOT_HPD when a pivot is not > 0.
 * Synchronizes the stream (the status has to be read back).  f32/f64. */
int elx_matrix_cholesky(int dtype, int device, int uplo, int64_t n, void* A, int64_t lda, void* stream);
/* El::TriangularInverse on Matrix<T> (src/lapack_like/funcs/Inverse/Triangular.cpp):
 * the n x n A := tri(A)^-1 in place on the uplo triangle; the other triangle, and
 * with ELX_UNIT the diagonal, is neither read nor written.  No singularity test (an
 * exact zero on a NON_UNIT diagonal leaves Inf / NaN).  Runs the blocked driver of
 * elx_triangular_inverse on the buffer, asynchronously on the stream.  f32/f64. */
int elx_matrix_triangular_inverse(int dtype, int device, int uplo, int diag, int64_t n, void* A, int64_t lda,
                                  void* stream);
/* El::Trtrmm on Matrix<T> (src/blas_like/level3/Trtrmm.cpp): the n x n A := L^T L
 * (ELX_LOWER) or U U^T (ELX_UPPER) in place on the uplo triangle; asynchronous on the
 * stream.  f32/f64. */
int elx_matrix_trtrmm(int dtype, int device, int uplo, int64_t n, void* A, int64_t lda, void* stream);
/* El::HPDInverse on Matrix<T> (src/lapack_like/funcs/Inverse/HPD.cpp): the n x n HPD
 * A := A^-1 in place on the uplo triangle (Cholesky, TriangularInverse, Trtrmm).
 * ELX_ERR_NOT_HPD as elx_matrix_cholesky; synchronizes the stream as it does.  f32/f64. */
int elx_matrix_hpd_inverse(int dtype, int device, int uplo, int64_t n, void* A, int64_t lda, void* stream);
/* El::LU on Matrix<T> (src/lapack_like/factor/LU.cpp): P A = L U of the m x n A in
 * place with partial pivoting; piv receives min(m, n) int32 entries in the matrix's
 * memory space, row j was swapped with row piv[j] (0-based).  ELX_ERR_SINGULAR when a
 * pivot is exactly zero (A and piv are then unspecified).  Synchronizes the stream
 * (the status has to be read back).  f32/f64. */
int elx_matrix_lu(int dtype, int device, int64_t m, int64_t n, void* A, int64_t lda, int32_t* piv, void* stream);
/* El::QR on Matrix<T> (src/lapack_like/factor/QR/Householder.hpp): A = Q R of the m x n
 * A in place by Householder reflections.  On return the upper trapezoid holds R with a
 * non-negative diagonal and the strict lower part the reflectors u_j (implicit leading
 * 1); tau and sig receive min(m, n) entries of the matrix's type in its memory space:
 * the Householder scalars and the signature (+-1), Q = H_0 .. H_{k-1} diag(sig), H_j =
 * I - tau_j [1; u_j][1; u_j]^T.  No failure mode; NaN and Inf propagate.  Does NOT
 * synchronize: on the GPU it is launches on the stream and nothing else.  f32/f64. */
int elx_matrix_qr(int dtype, int device, int64_t m, int64_t n, void* A, int64_t lda, void* tau, void* sig,
                  void* stream);
/* El::HermitianTridiag on Matrix<T> (src/lapack_like/condense/HermitianTridiag.cpp): Q^T A
 * Q = T in place on the uplo triangle of the n x n A; the other triangle is neither read
 * nor written.  tau receives n - 1 Householder scalars of the matrix's type in its memory
 * space.  ELX_LOWER: diag(A) and A(k+1, k) are T, A(k+2:n, k) the reflector of H_k (implicit
 * 1 at row k+1, scalar tau[k]).  ELX_UPPER: A(k-1, k) is the superdiagonal, A(0:k-1, k) the
 * reflector (implicit 1 at row k-1, scalar tau[k-1]).  A tail that is exactly zero gives
 * tau = 2.  No failure mode; NaN and Inf propagate.  Does NOT synchronize: on the GPU it is
 * launches on the stream and nothing else.  f32/f64. */
int elx_matrix_hermitian_tridiag(int dtype, int device, int uplo, int64_t n, void* A, int64_t lda, void* tau,
                                 void* stream);
/* ---- Level 2 on Matrix<T> (src/blas_like/level2): column-major A with any lda, vectors
 * with an element stride >= 1 (a row of a Matrix has stride ldim).  Asynchronous on the
 * stream; sums are kept in double (f64) or float (the other types) and rounded once; two
 * calls on the same input give the same bits.
 * El::Gemv: y := alpha op(A) x + beta y, A m x n.  beta == 0 overwrites y without reading
 * it; alpha == 0 or a zero-length x gives y := beta y without reading A or x.  All four types */
int elx_matrix_gemv(int dtype, int device, int orient, int64_t m, int64_t n, double alpha, const void* A, int64_t lda,
                    const void* x, int64_t incx, double beta, void* y, int64_t incy, void* stream);
/* El::Ger / El::Geru: A += alpha x y^T, A m x n.  f32/f64 */
int elx_matrix_ger(int dtype, int device, int64_t m, int64_t n, double alpha, const void* x, int64_t incx,
                   const void* y, int64_t incy, void* A, int64_t lda, void* stream);
/* El::Symv / El::Hemv: y := alpha A x + beta y with the symmetric n x n A given by its uplo
 * triangle; the other triangle is never read.  f32/f64 */
int elx_matrix_symv(int dtype, int device, int uplo, int64_t n, double alpha, const void* A, int64_t lda, const void* x,
                    int64_t incx, double beta, void* y, int64_t incy, void* stream);
/* symv::LocalColAccumulateL / U on one m x n block whose element (i, j) is the global
 * (i0 + i istride, j0 + j jstride): with ELX_LOWER (mirrored for ELX_UPPER)
 *   z_row[i] += alpha sum_{j: gj <= gi} a(i,j) x_col[j],  z_col[j] += alpha sum_{i: gi > gj} a(i,j) x_row[i];
 * x_row, z_row are indexed by local row, x_col, z_col by local column.  f32/f64 */
int elx_matrix_symv_accumulate(int dtype, int device, int uplo, int64_t m, int64_t n, double alpha, const void* A,
                               int64_t lda, const void* x_row, int64_t incxr, const void* x_col, int64_t incxc,
                               void* z_row, int64_t inczr, void* z_col, int64_t inczc, int64_t i0, int64_t istride,
                               int64_t j0, int64_t jstride, void* stream);
/* El::Syr / El::Her: A += alpha x x^T on the uplo triangle of the n x n A; the other
 * triangle is neither read nor written.  f32/f64 */
int elx_matrix_syr(int dtype, int device, int uplo, int64_t n, double alpha, const void* x, int64_t incx, void* A,
                   int64_t lda, void* stream);
/* El::Syr2 / El::Her2: A += alpha (x y^T + y x^T) likewise.  f32/f64 */
int elx_matrix_syr2(int dtype, int device, int uplo, int64_t n, double alpha, const void* x, int64_t incx,
                    const void* y, int64_t incy, void* A, int64_t lda, void* stream);

/* ---- BLAS-1 entrywise kernels (dtype-generic; scalars passed as double) --
 * Strides are element strides: X(i,j) = X[i*xcs + j*xrs].
 * axpy2d   replaces Axpy_GPU_impl            (src/hydrogen/blas/gpu/Axpy.cu:119-189)
 * copy2d   replaces Copy_GPU_impl            (src/hydrogen/blas/gpu/Copy.cu:104-205)
 * transpose replaces Transpose_GPU_impl      (src/hydrogen/blas/gpu/Transpose.cu:102-127)
 * scale2d  replaces Scale_GPU_impl           (src/hydrogen/blas/gpu/Scale.cu:45-81)
 * fill2d   replaces Fill_GPU_impl            (src/hydrogen/blas/gpu/Fill.cu:55-76)
 * hadamard replaces Hadamard_GPU_impl        (src/hydrogen/blas/gpu/Hadamard.cu:62-117)
 * entrywise_map replaces EntrywiseMapImpl    (include/hydrogen/blas/gpu/EntrywiseMapImpl.hpp:36-211) */
int elx_axpy2d(int dtype, int64_t m, int64_t n, double alpha,
               const void* X, int64_t xcs, int64_t xrs,
               void* Y, int64_t ycs, int64_t yrs, void* stream);
/* pack / unpack of redistribution portions (include/El/blas_like/level1/Copy/util.hpp),
 * each ONE batched strided-copy launch over every portion; device = ELX_DEVICE_*.
 * Portion k + l*colStride holds rows Shift_(k,colAlign,colStride) + i*colStride
 * and columns Shift_(l,rowAlign,rowStride) + j*rowStride, column-major with ld =
 * its height; portionSize (elements) must hold the largest portion.
 *   elx_pack_strided:   StridedPack (util.hpp:667-691); rowStride = 1 is
 *                       ColStridedPack (:359-378), colStride = 1 RowStridedPack (:148-166)
 *   elx_unpack_strided: StridedUnpack (:694-718) / ColStridedUnpack / RowStridedUnpack
 *   elx_pack_partial_strided / elx_unpack_partial_strided: PartialColStrided*
 *                       (cols = 1, util.hpp:460-552) and PartialRowStrided* (cols = 0,
 *                       :186-230); stride = strideUnion * stridePart, shiftA/B = the
 *                       local matrix's own shift on the partial lattice
 *   elx_unpack_axpy_strided: the fused reduce-scatter epilogue, B += alpha * portion
 *                       (axpy::util::InterleaveMatrixUpdate, Axpy/util.hpp:23-50) */
int elx_pack_strided(int device, int dtype, int64_t height, int64_t width,
                     int64_t colAlign, int64_t colStride, int64_t rowAlign, int64_t rowStride,
                     const void* A, int64_t lda, void* portions, int64_t portionSize, void* stream);
int elx_unpack_strided(int device, int dtype, int64_t height, int64_t width,
                       int64_t colAlign, int64_t colStride, int64_t rowAlign, int64_t rowStride,
                       const void* portions, int64_t portionSize, void* B, int64_t ldb, void* stream);
int elx_pack_partial_strided(int device, int dtype, int cols, int64_t height, int64_t width,
                             int64_t align, int64_t stride, int64_t strideUnion, int64_t stridePart,
                             int64_t rankPart, int64_t shiftA, const void* A, int64_t lda,
                             void* portions, int64_t portionSize, void* stream);
int elx_unpack_partial_strided(int device, int dtype, int cols, int64_t height, int64_t width,
                               int64_t align, int64_t stride, int64_t strideUnion, int64_t stridePart,
                               int64_t rankPart, int64_t shiftB, const void* portions,
                               int64_t portionSize, void* B, int64_t ldb, void* stream);
int elx_unpack_axpy_strided(int device, int dtype, int64_t height, int64_t width, double alpha,
                            int64_t colAlign, int64_t colStride, int64_t rowAlign, int64_t rowStride,
                            const void* portions, int64_t portionSize, void* B, int64_t ldb,
                            void* stream);
int elx_copy2d(int dtype, int64_t m, int64_t n,
               const void* A, int64_t acs, int64_t ars,
               void* B, int64_t bcs, int64_t brs, void* stream);
/* type-converting copy2d: B(i,j) = (dst_dtype) A(i,j), one round-to-nearest-even
 * from the exact source value; replaces the SrcT != DestT instantiations of
 * Copy_GPU_impl (src/hydrogen/blas/gpu/Copy.cu:93-205, ETI :207-244) */
int elx_copy2d_convert(int src_dtype, int dst_dtype, int64_t m, int64_t n,
                       const void* A, int64_t acs, int64_t ars,
                       void* B, int64_t bcs, int64_t brs, void* stream);
int elx_transpose(int dtype, int64_t m, int64_t n,
                  const void* A, int64_t lda, void* B, int64_t ldb, void* stream);
int elx_scale2d(int dtype, int64_t m, int64_t n, double alpha,
                void* A, int64_t lda, void* stream);
int elx_fill2d(int dtype, int64_t m, int64_t n, double value,
               void* A, int64_t lda, void* stream);
int elx_hadamard2d(int dtype, int64_t m, int64_t n,
                   const void* A, int64_t lda, const void* B, int64_t ldb,
                   void* C, int64_t ldc, void* stream);
int elx_entrywise_map(int dtype, int fn, int64_t m, int64_t n,
                      const void* A, int64_t lda, void* B, int64_t ldb, void* stream);
/* replaces CombineImpl (include/hydrogen/blas/gpu/CombineImpl.hpp:47-213) */
int elx_combine(int dtype, int fn, int64_t m, int64_t n,
                const void* A, int64_t lda, void* B, int64_t ldb, void* stream);
/* grid-independent synthetic fill: A(i,j) = center + radius*u(seed,i0+i,j0+j), u in [-1,1) */
int elx_fill_hash(int dtype, int64_t m, int64_t n, void* A, int64_t lda,
                  int64_t i0, int64_t istride, int64_t j0, int64_t jstride,
                  uint64_t seed, double center, double radius, void* stream);

/* ---- communication: replaces El::mpi::{AllGather,ReduceScatter,AllToAll,
 * SendRecv,Broadcast,Barrier} + Aluminum (src/core/imports/mpi/{AllGather,ReduceScatter,...}.hpp,
 * include/El/core/imports/aluminum.hpp:24-365).  Backend: RCCL over xGMI for
 * device buffers, or a caller-supplied host collective (e.g. a gloo bridge). */
typedef struct elx_comm_s* elx_comm_t;
#define ELX_COLL_ALLGATHER      0  /* recv[r*count..] = send of rank r           */
#define ELX_COLL_REDUCE_SCATTER 1  /* recv = sum_r send_r[me*count..]           */
#define ELX_COLL_ALLTOALL       2  /* recv[r*count..] = send_r[me*count..]      */
#define ELX_COLL_SENDRECV       3  /* send -> peer, recv <- peer2               */
#define ELX_COLL_BCAST          4  /* buffer (send==recv) from root=peer        */
#define ELX_COLL_ALLREDUCE      5  /* recv = sum_r send_r                        */
#define ELX_COLL_BARRIER        6
/* host collective callback; count is in ELEMENTS of dtype, buffers are host
 * memory, `group` is an opaque id returned by the split callback (0 = world). */
typedef int (*elx_host_coll_fn)(void* ctx, int op, int group, int dtype,
                                const void* send, void* recv, int64_t count,
                                int peer, int peer2);
/* host split callback: collective over `group` (the library only splits the
 * world, group 0); returns the new group's id, this rank's rank and its size */
typedef int (*elx_host_split_fn)(void* ctx, int group, int color, int key,
                                 int* out_group, int* out_rank, int* out_size);
int elx_comm_unique_id(unsigned char id[128]);
int elx_comm_init_rccl(elx_comm_t* world, int rank, int size, const unsigned char id[128]);
int elx_comm_init_host(elx_comm_t* world, int rank, int size,
                       elx_host_coll_fn coll, elx_host_split_fn split, void* ctx);
/* Grid(mpi::Comm) from a communicator the caller already owns: borrow an
 * existing RCCL communicator (ncclComm_t passed as void*; never destroyed by
 * the library, its grid splits are) */
int elx_comm_wrap_rccl(elx_comm_t* comm, void* nccl_comm);
int elx_comm_rank(elx_comm_t comm, int* rank);
int elx_comm_size(elx_comm_t comm, int* size);
int elx_comm_destroy(elx_comm_t comm);
/* El::mpi::COMM_WORLD (include/El/core/imports/mpi.hpp:86): the library's world
 * communicator, size 1 until elx_initialize() builds one from the launcher's
 * environment or the caller installs one.  elx_comm_world returns a BORROWED
 * handle (never pass it to elx_comm_destroy); elx_comm_set_world shares the
 * given communicator (the caller may destroy its own handle afterwards). */
int elx_comm_world(elx_comm_t* comm);
int elx_comm_set_world(elx_comm_t comm);
/* byte broadcast from rank 0 over TCP (rank 0 listens on `port`): the unique-id
 * exchange for RCCL worlds started without MPI */
int elx_rendezvous_bcast(void* data, size_t bytes, int rank, int size, const char* addr, int port,
                         double timeout_s);
/* stage watchdog: arms a deadline (seconds > 0) for the named stage and prints
 * "[elx] stage <name>" to stderr; on overrun, or an asynchronous RCCL error on
 * an owned communicator, every owned RCCL communicator is aborted and the
 * process exits with status ELX_WATCHDOG_EXIT naming the stage.  seconds <= 0
 * disarms. */
#define ELX_WATCHDOG_EXIT 75
int elx_watchdog_stage(const char* name, double seconds);
/* text the watchdog writes to stdout before it exits (NULL / "": nothing), and
 * the exit status it then uses (ELX_WATCHDOG_EXIT until set) — e.g. a
 * benchmark's result line already measured when a later, optional stage hangs */
int elx_watchdog_epitaph(const char* text, int exit_code);
/* raw typed collectives on device (RCCL) or host (callback) buffers, on `stream` */
int elx_comm_allgather(elx_comm_t comm, int dtype, const void* send, void* recv,
                       int64_t count, void* stream);
int elx_comm_reduce_scatter(elx_comm_t comm, int dtype, const void* send, void* recv,
                            int64_t count, void* stream);
int elx_comm_barrier(elx_comm_t comm);
/* the rest of El::mpi's typed collectives (src/core/imports/mpi/{AllReduce,
 * Broadcast.hpp:11-107, AllToAll.hpp:11-105, SendRecv.hpp:9-60}, mpi.cpp:438-441
 * for Split): counts in elements; RCCL comms take device buffers on `stream`,
 * host comms host buffers */
int elx_comm_split(elx_comm_t comm, int color, int key, elx_comm_t* out);
int elx_comm_allreduce(elx_comm_t comm, int dtype, const void* send, void* recv,
                       int64_t count, void* stream);
int elx_comm_bcast(elx_comm_t comm, int dtype, void* buf, int64_t count, int root,
                   void* stream);
int elx_comm_alltoall(elx_comm_t comm, int dtype, const void* send, void* recv,
                      int64_t count, void* stream);
int elx_comm_sendrecv(elx_comm_t comm, int dtype, const void* send, int dest,
                      void* recv, int src, int64_t count, void* stream);
/* El::mpi's typed collectives with the buffers' device explicit (what
 * El::mpi::*(..., SyncInfo<D>) binds; include/El/core/imports/mpi.hpp:593-633
 * SendRecv, :675-720 Broadcast, :861-930 AllGather, :1006-1075 AllToAll,
 * :1248-1351 AllReduce, :1361- ReduceScatter).  device = ELX_DEVICE_GPU: device
 * buffers, enqueued on `stream` (RCCL) or staged (host backend);
 * ELX_DEVICE_CPU: host buffers, synchronous (staged through device memory on an
 * RCCL communicator).  op: the El::mpi::Op of the reduction. */
#define ELX_OP_SUM  0
#define ELX_OP_PROD 1
#define ELX_OP_MAX  2
#define ELX_OP_MIN  3
int elx_mpi_allgather(elx_comm_t comm, int dtype, int device, const void* send, void* recv, int64_t count,
                      void* stream);
int elx_mpi_reduce_scatter(elx_comm_t comm, int dtype, int device, int op, const void* send, void* recv,
                           int64_t count, void* stream);
int elx_mpi_allreduce(elx_comm_t comm, int dtype, int device, int op, const void* send, void* recv,
                      int64_t count, void* stream);
int elx_mpi_alltoall(elx_comm_t comm, int dtype, int device, const void* send, void* recv, int64_t count,
                     void* stream);
int elx_mpi_bcast(elx_comm_t comm, int dtype, int device, void* buf, int64_t count, int root, void* stream);
int elx_mpi_sendrecv(elx_comm_t comm, int dtype, int device, const void* send, int64_t send_count, int dest,
                     void* recv, int64_t recv_count, int src, void* stream);
/* cumulative traffic counters of the collectives issued by this process */
int elx_comm_stats(int64_t* bytes_moved, double* seconds, int64_t* calls);
int elx_comm_stats_reset(void);

/* ---- El::Grid (src/core/Grid.cpp:58-206) --------------------------------- */
typedef struct elx_grid_s* elx_grid_t;
int elx_grid_default_height(int size);                 /* Grid::DefaultHeight */
int elx_grid_create(elx_grid_t* grid, elx_comm_t world, int height, int order);
/* info[0..7] = height, width, size, rank(VC), mcRank, mrRank, vcRank, vrRank */
int elx_grid_info(elx_grid_t grid, int* info);
int elx_grid_destroy(elx_grid_t grid);

/* ---- El::DistMatrix<T,U,V,ELEMENT,D> (include/El/core/DistMatrix/, src/core/DistMatrix/) */
typedef struct elx_dm_s* elx_dm_t;
int elx_dm_create(elx_dm_t* A, elx_grid_t grid, int dtype, int coldist, int rowdist,
                  int device, int root);
int elx_dm_destroy(elx_dm_t A);
int elx_dm_align(elx_dm_t A, int colAlign, int rowAlign, int constrain);
int elx_dm_align_with(elx_dm_t A, elx_dm_t B, int constrain);
int elx_dm_resize(elx_dm_t A, int64_t height, int64_t width);
/* info[0..12] = height, width, localHeight, localWidth, ldim, colAlign, rowAlign,
 *               colShift, rowShift, colStride, rowStride, participating, viewing */
int elx_dm_info(elx_dm_t A, int64_t* info);
int elx_dm_buffer(elx_dm_t A, void** ptr);
/* host <-> local buffer (column-major, leading dim ld) */
int elx_dm_set_local(elx_dm_t A, const void* host, int64_t ld);
int elx_dm_get_local(elx_dm_t A, void* host, int64_t ld);
/* El::FrobeniusNorm (collective over the grid; each entry counted once) */
int elx_dm_frobenius_norm(elx_dm_t A, double* out);
/* V := A(i0:i1, j0:j1) (a view, El::View / A(IR,IR)) */
int elx_dm_view(elx_dm_t* V, elx_dm_t A, int64_t i0, int64_t i1, int64_t j0, int64_t j1);
/* A views caller storage as its local block: ElementalMatrix::Attach
 * (src/core/DistMatrix/ElementMatrix.cpp:368-409).  Alignments become
 * constrained, the caller keeps ownership, ldim >= max(localHeight, 1). */
int elx_dm_attach(elx_dm_t A, int64_t height, int64_t width, int colAlign, int rowAlign,
                  void* buffer, int64_t ldim, int root);
/* B := A  (DistMatrix::operator=, the redistribution dispatch table,
 * src/core/DistMatrix/ElementMatrix/{MC_MR,MC_STAR,...}.cpp); bit-exact.
 * Different element types: El::Copy(ElementalMatrix<S>, DistMatrix<T>)
 * (include/El/blas_like/level1/CopyDistMatrix.hpp:28-57) — redistribute in S
 * to B's distribution and alignment, then convert locally (elx_copy2d_convert). */
int elx_dm_copy(elx_dm_t B, elx_dm_t A);
/* B := A^T (El::Transpose, include/El/blas_like/level1/Transpose.hpp:191-250) */
int elx_dm_transpose(elx_dm_t A, elx_dm_t B);
/* synthetic grid-independent fill from global indices (see elx_fill_hash) */
int elx_dm_fill_hash(elx_dm_t A, uint64_t seed, double center, double radius);
/* El::InitializeRandom(deterministic) (src/core/random.cpp:24-35): seed the
 * process-global mt19937 with (secs << 16) | worldRank, secs = 21 if deterministic */
int elx_initialize_random(int deterministic, int world_rank);
/* El::Uniform / MakeUniform (src/matrices/random/independent/Uniform.cpp:18-66):
 * the reference's draws, bit for bit, for the same grid and call order */
int elx_dm_uniform(elx_dm_t A, int64_t height, int64_t width, double center, double radius);
int elx_dm_make_uniform(elx_dm_t A, double center, double radius);
int elx_dm_synchronize(elx_dm_t A);
/* El::Write / El::Read (src/io/Write.cpp:70-86, src/io/Read.cpp:71-120) in the
 * reference's BINARY ([Int h][Int w][column-major data], file basename.bin)
 * and BINARY_FLAT (data only, basename.dat; Read takes the size from A)
 * formats; int_bytes = sizeof(El::Int) of the reference build (4 by default,
 * 8 with Hydrogen_USE_64BIT_INTS); f16/bf16 travel as float like the
 * reference's gpu_half_type overloads.  Read with ELX_FILE_AUTO detects the
 * format from the extension. */
#define ELX_FILE_AUTO        0
#define ELX_FILE_BINARY      3
#define ELX_FILE_BINARY_FLAT 4
int elx_dm_write(elx_dm_t A, const char* basename, int format, int int_bytes);
int elx_dm_read(elx_dm_t A, const char* filename, int format, int int_bytes);
/* El::SetSyncInfo / SyncInfoFromMatrix (include/El/core/Matrix/decl.hpp:523-535,
 * impl_gpu.hpp:509-513): move the matrix's work to `stream` (ordered after the
 * work already queued on its old stream; the local buffer is then released on
 * the new one) / query it.  A no-op / NULL for CPU matrices. */
int elx_dm_set_stream(elx_dm_t A, void* stream);
int elx_dm_stream(elx_dm_t A, void** stream);

/* DistMatrix::Get (ElementMatrix/setup.hpp:463-490): collective over the grid,
 * every rank returns A(i,j) (16-bit values widened exactly to double).
 * Set / Update (setup.hpp:552-604): each rank holding (i,j) writes its copy;
 * not collective.  Fill (Fill.hpp:20-70): every entry := value. */
int elx_dm_get(elx_dm_t A, int64_t i, int64_t j, double* value);
int elx_dm_set(elx_dm_t A, int64_t i, int64_t j, double value);
int elx_dm_update(elx_dm_t A, int64_t i, int64_t j, double value);
int elx_dm_fill(elx_dm_t A, double value);

/* ---- distributed BLAS-1 front doors (include/El/blas_like/level1/) ---- */
int elx_dm_axpy(double alpha, elx_dm_t X, elx_dm_t Y);       /* Axpy.hpp:151-176     */
int elx_dm_scale(double alpha, elx_dm_t A);                   /* Scale.hpp:18-31      */
int elx_dm_zero(elx_dm_t A);                                  /* Zero.hpp             */
int elx_dm_hadamard(elx_dm_t A, elx_dm_t B, elx_dm_t C);      /* Hadamard.hpp:107-131 */
int elx_dm_entrywise_map(int fn, elx_dm_t A, elx_dm_t B);     /* EntrywiseMap.hpp:90-137 */
int elx_dm_combine(int fn, elx_dm_t A, elx_dm_t B);           /* EntrywiseMap.hpp:187-202, per local block */
/* reduce-scatter family: B += alpha * contract(A)  (AxpyContract.hpp:483-544) */
int elx_dm_axpy_contract(double alpha, elx_dm_t A, elx_dm_t B);

/* ---- Level 3: El::Gemm / El::LocalGemm (src/blas_like/level3/Gemm.cpp:273-426) */
int elx_gemm(int orientA, int orientB, double alpha, elx_dm_t A, elx_dm_t B,
             double beta, elx_dm_t C, int alg);
int elx_local_gemm(int orientA, int orientB, double alpha, elx_dm_t A, elx_dm_t B,
                   double beta, elx_dm_t C);
/* El::Syrk / El::Herk on DistMatrices (src/blas_like/level3/Syrk.cpp:196-225,
 * Herk.cpp): C := alpha op(A) op(A)^T + beta C on C's uplo triangle only; the
 * other triangle is neither read nor written.  conjugate (Herk) is a no-op for
 * the real types. */
int elx_syrk(int uplo, int orient, double alpha, elx_dm_t A, double beta, elx_dm_t C, int conjugate);
/* El::Trrk (src/blas_like/level3/Trrk.cpp:100-117): C := alpha op(A) op(B) + beta C
 * on C's uplo triangle only */
int elx_trrk(int uplo, int orientA, int orientB, double alpha, elx_dm_t A, elx_dm_t B,
             double beta, elx_dm_t C);
/* El::Syr2k / El::Her2k (src/blas_like/level3/Syr2k.cpp:78-105, Her2k.cpp):
 * C := alpha (op(A) op(B)^T + op(B) op(A)^T) + beta C on C's uplo triangle */
int elx_syr2k(int uplo, int orient, double alpha, elx_dm_t A, elx_dm_t B, double beta,
              elx_dm_t C, int conjugate);
/* El::Trsm on DistMatrices (src/blas_like/level3/Trsm.cpp:129-420): B := alpha
 * op(A)^-1 B (ELX_LEFT) or alpha B op(A)^-1 (ELX_RIGHT); float and double */
int elx_trsm(int side, int uplo, int orient, int diag, double alpha, elx_dm_t A, elx_dm_t B,
             int checkIfSingular);  /* ELX_ERR_SINGULAR on an exact zero NON_UNIT diagonal (Trsm.cpp:60-68) */
/* El::Trmm on DistMatrices (src/blas_like/level3/Trmm.cpp:53-89): B := alpha
 * op(tri(A)) B (ELX_LEFT) or alpha B op(tri(A)) (ELX_RIGHT), in place; float and double */
int elx_trmm(int side, int uplo, int orient, int diag, double alpha, elx_dm_t A, elx_dm_t B);
/* El::Cholesky on a DistMatrix (src/lapack_like/factor/Cholesky/LowerVariant3.hpp:78-134):
 * A := its Cholesky factor in place on the uplo triangle; ELX_ERR_NOT_HPD (on every
 * rank) when a pivot is not > 0; float and double */
int elx_cholesky(int uplo, elx_dm_t A);
/* the largest diagonal block one leaf kernel factors (kPotrfMax): elx_cholesky blocks by
 * min(Blocksize(), this) */
int64_t elx_cholesky_leaf_max(void);
/* El::cholesky::SolveAfter (Cholesky/SolveAfter.hpp:78-107): B := A^-1 B from the
 * factor that elx_cholesky left in A's uplo triangle */
int elx_cholesky_solve_after(int uplo, int orient, elx_dm_t A, elx_dm_t B);
/* El::TriangularInverse on a DistMatrix (src/lapack_like/funcs/Inverse/Triangular.cpp):
 * A := tri(A)^-1 in place on the uplo triangle (ELX_UNIT: the diagonal is neither read
 * nor written); no singularity test; float and double */
int elx_triangular_inverse(int uplo, int diag, elx_dm_t A);
/* El::Trtrmm on a DistMatrix (src/blas_like/level3/Trtrmm.cpp): A := L^T L (ELX_LOWER)
 * or U U^T (ELX_UPPER) in place on the uplo triangle; conjugate changes nothing for the
 * real types; float and double */
int elx_trtrmm(int uplo, elx_dm_t A, int conjugate);
/* El::HPDInverse on a DistMatrix (src/lapack_like/funcs/Inverse/HPD.cpp): A := A^-1 in
 * place on the uplo triangle; ELX_ERR_NOT_HPD (on every rank) from the Cholesky stage,
 * which leaves A as the failed factorization left it; float and double */
int elx_hpd_inverse(int uplo, elx_dm_t A);
/* El::Permutation / El::DistPermutation as a swap sequence (rows k and dest[k] swapped
 * for k = 0, 1, ...: the LAPACK ipiv, 0-based).  The sequence lives in host memory for
 * ELX_DEVICE_CPU and in device memory for ELX_DEVICE_GPU; elx_lu resets it to A's
 * height and device.  elx_perm_swaps copies the elx_perm_num_swaps destinations to a
 * host array (synchronizing the permutation's stream).  elx_perm_permute_rows:
 * B := P B (inverse = 0) or P^-1 B, bit-exact, any grid; float and double. */
typedef struct elx_perm_s* elx_perm_t;
int elx_perm_create(elx_perm_t* P);
int elx_perm_destroy(elx_perm_t P);
int elx_perm_make_identity(elx_perm_t P, int64_t n, int device);
int64_t elx_perm_height(elx_perm_t P);
int64_t elx_perm_num_swaps(elx_perm_t P);
int elx_perm_swaps(elx_perm_t P, int64_t* dests);
int elx_perm_permute_rows(elx_perm_t P, elx_dm_t B, int inverse);
/* El::LU with partial pivoting (src/lapack_like/factor/LU.cpp:88-131): P A = L U in
 * place, L unit lower and U upper, min(m, n) swaps in P.  ELX_ERR_SINGULAR (on every
 * rank; the message names the 1-based column) when a pivot is exactly zero; A and P
 * are then unspecified.  float and double */
int elx_lu(elx_dm_t A, elx_perm_t P);
/* El::lu::SolveAfter (LU/SolveAfter.hpp:94-121): B := op(A)^-1 B from elx_lu's A and P */
int elx_lu_solve_after(int orient, elx_dm_t A, elx_perm_t P, elx_dm_t B);
/* El::LinearSolve (src/lapack_like/solve/Linear.cpp): B := A^-1 B; A is left as it was */
int elx_linear_solve(elx_dm_t A, elx_dm_t B);
/* the leaf kernel's panel width and its rows per workgroup (kGetrfLeafCols, kGetrfLeafRows) */
int64_t elx_lu_leaf_cols(void);
int64_t elx_lu_leaf_rows(void);
/* El::QR (src/lapack_like/factor/QR/Householder.hpp): A = Q R in place; t and d (any
 * distribution) are resized to min(m, n) x 1 and receive the Householder scalars and
 * the signature (+-1); R has a non-negative diagonal.  float and double */
int elx_qr(elx_dm_t A, elx_dm_t t, elx_dm_t d);
/* El::qr::ApplyQ (QR/ApplyQ.hpp): B := Q B (ELX_NORMAL) or Q^T B from elx_qr's A, t and
 * d.  side must be ELX_LEFT (ELX_ERR_LOGIC otherwise) */
int elx_qr_apply_q(int side, int orient, elx_dm_t A, elx_dm_t t, elx_dm_t d, elx_dm_t B);
/* El::qr::SolveAfter (QR/SolveAfter.hpp), m >= n: ELX_NORMAL X := argmin ||A X - B||_F;
 * ELX_TRANSPOSE / ELX_ADJOINT the minimum-norm X with A^T X = B */
int elx_qr_solve_after(int orient, elx_dm_t A, elx_dm_t t, elx_dm_t d, elx_dm_t B, elx_dm_t X);
/* El::qr::Explicit: A := the thin Q (m x k), R := the k x n upper trapezoid */
int elx_qr_explicit(elx_dm_t A, elx_dm_t R);
/* El::qr::ExplicitTriang: A := R */
int elx_qr_explicit_triang(elx_dm_t A);
/* El::LeastSquares (src/lapack_like/euclidean_min/LeastSquares.cpp) for m >= n; A is
 * left as it was.  m < n is ELX_ERR_UNSUPPORTED */
int elx_least_squares(int orient, elx_dm_t A, elx_dm_t B, elx_dm_t X);
/* the QR leaf kernel's panel width and its rows per workgroup (kGeqrfLeafCols, kGeqrfLeafRows) */
int64_t elx_qr_leaf_cols(void);
int64_t elx_qr_leaf_rows(void);
/* El::HermitianTridiag (src/lapack_like/condense/HermitianTridiag.cpp): A := the condensed
 * form on its uplo triangle, t (any distribution) is resized to (n - 1) x 1 and receives
 * the Householder scalars.  A grid of more than one process runs the right-looking loop over
 * elx_blocksize on A [MC,MR]; only the last block is staged [*,*].  float and double */
int elx_hermitian_tridiag(int uplo, elx_dm_t A, elx_dm_t t);
/* El::herm_tridiag::ApplyQ: B := Q B (ELX_NORMAL) or Q^T B from elx_hermitian_tridiag's A
 * and t.  side must be ELX_LEFT (ELX_ERR_LOGIC otherwise) */
int elx_hermitian_tridiag_apply_q(int side, int uplo, int orient, elx_dm_t A, elx_dm_t t, elx_dm_t B);
/* El::herm_tridiag::ExplicitCondensed: the reduction, then zero outside the three
 * diagonals on the uplo side */
int elx_hermitian_tridiag_explicit_condensed(int uplo, elx_dm_t A);
/* the local driver's panel width (kSytrdPanelCols = 32 unless elx_set_tridiag_panel_cols
 * changed it) and the panel kernels' rows per workgroup (kSytrdRows).  The setter takes 1 ..
 * 64, or 0 for the default; it exists for the width measurement in tools/tridiag_bench.py.
 * The environment variable ELX_TRIDIAG_PANEL=level2, read at every call, selects the panel
 * composed from the Level-2 routines instead of the fused kernels (the timing baseline) */
int64_t elx_tridiag_panel_cols(void);
int elx_set_tridiag_panel_cols(int64_t w);
int64_t elx_tridiag_rows(void);
/* ---- Level 2 on DistMatrices (src/blas_like/level2).  A vector is an n x 1 or a 1 x n
 * DistMatrix of any distribution; A of another distribution than [MC,MR] goes through a
 * [MC,MR] copy.  Real types: `conjugate` is accepted and changes nothing (Hemv = Symv,
 * Her = Syr, Her2 = Syr2, Geru = Ger).  Nonconformal operands, mixed types, devices or
 * grids are ELX_ERR_LOGIC.
 * El::Gemv (Gemv/Normal.hpp, Gemv/Transpose.hpp): y := alpha op(A) x + beta y.  All four types */
int elx_gemv(int orient, double alpha, elx_dm_t A, elx_dm_t x, double beta, elx_dm_t y);
/* the beta-less overload: y is aligned with A, resized to a column vector and zeroed first */
int elx_gemv_resize(int orient, double alpha, elx_dm_t A, elx_dm_t x, elx_dm_t y);
/* El::LocalGemv on operands already spread and aligned with A [MC,MR]: ELX_NORMAL takes x
 * [MR,*] or [*,MR] and y [MC,*] or [*,MC]; ELX_TRANSPOSE / ELX_ADJOINT the two exchanged */
int elx_local_gemv(int orient, double alpha, elx_dm_t A, elx_dm_t x, double beta, elx_dm_t y);
/* El::Ger / El::Geru (Ger.cpp): A += alpha x y^T.  float and double */
int elx_ger(double alpha, elx_dm_t x, elx_dm_t y, elx_dm_t A);
/* El::Symv / El::Hemv (Symv.cpp): y := alpha A x + beta y, A symmetric with only its uplo
 * triangle read.  float and double */
int elx_symv(int uplo, double alpha, elx_dm_t A, elx_dm_t x, double beta, elx_dm_t y, int conjugate);
/* El::symv::LocalColAccumulate (Symv/L.hpp, Symv/U.hpp) on the local block of A [MC,MR]:
 * z[MC,*] += alpha tri(A) x[MR,*] and z[MR,*] += alpha tri'(A)^T x[MC,*], tri the uplo
 * triangle with and tri' without the diagonal; all four vectors are columns aligned with A */
int elx_symv_local_col_accumulate(int uplo, double alpha, elx_dm_t A, elx_dm_t x_MC_STAR, elx_dm_t x_MR_STAR,
                                  elx_dm_t z_MC_STAR, elx_dm_t z_MR_STAR, int conjugate);
/* El::Syr / El::Her (Syr.cpp): A += alpha x x^T on the uplo triangle.  float and double */
int elx_syr(int uplo, double alpha, elx_dm_t x, elx_dm_t A, int conjugate);
/* El::Syr2 / El::Her2 (Syr2.cpp): A += alpha (x y^T + y x^T) on the uplo triangle.  float and double */
int elx_syr2(int uplo, double alpha, elx_dm_t x, elx_dm_t y, elx_dm_t A, int conjugate);
/* the Level-2 kernels' launch shapes: rows of A per workgroup of the A x kernel (also the
 * row chunk in which the A^T x kernel splits its sum), columns per x chunk of the A x kernel
 * (also the chunk in which it splits its sum), and the Symv kernel's square tile */
int64_t elx_level2_gemv_rows(void);
int64_t elx_level2_gemv_cols(void);
int64_t elx_level2_symv_tile(void);
/* how many ranges the summed dimension of an m x n Gemv is cut into on the GPU (1: one
 * launch; more: partial sums in workspace and a fixed-order second launch) */
int64_t elx_level2_gemv_splits(int orient, int64_t m, int64_t n);
/* El::Symm / El::Hemm (src/blas_like/level3/Symm.cpp:55-80): C := alpha A B + beta C
 * (ELX_LEFT) or alpha B A + beta C (ELX_RIGHT); A symmetric, only its uplo triangle read */
int elx_symm(int side, int uplo, double alpha, elx_dm_t A, elx_dm_t B, double beta, elx_dm_t C,
             int conjugate);
/* A := alpha A on its uplo trapezoid (include/El/blas_like/level1/ScaleTrapezoid.hpp:47-88) */
int elx_dm_scale_trapezoid(double alpha, int uplo, elx_dm_t A, int64_t offset);
/* Blocksize stack (src/blas_like/blocksizes.cpp:38-72; environment.cpp:314-315
 * leaves one entry, 128).  elx_blocksize returns -1 on an empty stack (error
 * text in elx_last_error). */
int elx_set_blocksize(int64_t nb);
int64_t elx_blocksize(void);
int elx_push_blocksize(int64_t nb);
int elx_pop_blocksize(void);
int elx_empty_blocksize_stack(void);
/* El::Initialize / El::Finalize (src/core/environment.cpp:215-330,337-372):
 * world communicator from RANK / WORLD_SIZE / LOCAL_RANK / MASTER_ADDR (RCCL,
 * unique id over elx_rendezvous_bcast on ELX_RENDEZVOUS_PORT, default
 * MASTER_PORT + 1; size 1 without them), blocksize stack reset to {128}, the
 * deterministic RNG seeded (21<<16)|rank.  Finalize drops the world and
 * empties the blocksize stack. */
int elx_initialize(void);
int elx_finalize(void);
/* compute panel: how many communicated panels are fused into one local MFMA
 * update (0 = automatic). Changes only the summation order (normwise tol). */
int elx_set_compute_panel(int64_t kpanel);
/* algorithm the last elx_gemm call actually ran (after the heuristic) */
int elx_last_gemm_algorithm(void);
/* stream pool of the multistream (_MS) variants: hydrogen::SyncInfoPool and
 * H_STREAMPOOL_SIZE (src/blas_like/level3/SyncInfoPool.hpp:23-195, Gemm.cpp:17-90).
 * n > 1: GEMM_DEFAULT on GPU matrices picks SUMMA_{A,B,C}_MS and panels run on
 * n streams with duplicated RCCL communicators; 0 = read H_STREAMPOOL_SIZE */
int elx_set_stream_pool_size(int n);
int elx_stream_pool_size(void);
/* Profiling (replaces AUTO_PROFILE_REGION/NVTX ranges, include/El/core/Profiling.hpp:143-264):
 * when on, every local MFMA update and every panel transfer issued by the SUMMA
 * drivers is bracketed by HIP events on the stream it runs on.  stats: summed
 * kernel ms, launches, algorithmic FLOPs; summed transfer ms and bytes moved. */
int elx_set_profiling(int on);
int elx_profile_stats(double* gemm_ms, int64_t* gemm_launches, double* gemm_flops,
                      double* comm_ms, int64_t* comm_bytes);
/* transfer-only timing of the RCCL exchanges (events around each grouped
 * send/recv on its stream, pack/unpack excluded): summed ms, bytes received */
int elx_profile_transfers(double* transfer_ms, int64_t* bytes, int64_t* transfers);
/* compute-stream idle time between consecutive SUMMA panel updates (what the
 * panel pipeline failed to hide), summed over the profiled calls */
int elx_profile_pipeline(double* gap_ms, int64_t* gaps);

#ifdef __cplusplus
}
#endif
#endif /* ELEMENTAL_AMD_H */
