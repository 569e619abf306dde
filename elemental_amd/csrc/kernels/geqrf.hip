// Householder QR of one tall column panel: the leaf of LocalQR (qr::PanelHouseholder,
// src/lapack_like/factor/QR/PanelHouseholder.hpp, with reflector::Col; the
// reference's GPU build has no QR panel of its own).
//
// A leaf is m x w, w <= kGeqrfLeafCols, column-major, m arbitrary (m < w included;
// k = min(m, w) reflectors).  The norm of column j and its dot products with the
// columns to its right involve every row, so, as in getrf.hip, the leaf is spread
// over ceil(m / R) workgroups of R = kGeqrfLeafRows threads, one thread per row,
// and the global dependency is a KERNEL BOUNDARY: one launch per column step.  No
// grid-wide barrier, no flags, no spinning, no status word, nothing read back.
//
//   geqrf_step_kernel(j)  reads what launch j - 1 left in scratch under parity
//       j & 1: per workgroup the scaled norm pair (mx, sum (a/mx)^2) of column j
//       over rows > j, the dots sum (a(i,j)/mx) a(i,c) for c > j over the same
//       rows, and a copy of row j in columns j..w-1 (written by the workgroup that
//       owns the row: that row is rewritten during launch j, so nobody else may
//       read it from A).  Every workgroup combines the partials in the same fixed
//       order (so all of them, and every run, get the same bits): M = max mx,
//       nu = M sqrt(sum ssq (mx/M)^2), dot_c / M = sum pdot_c (mx/M).  Then, with
//       alpha = a(j,j):
//         nu == 0:   t = 2, beta = -alpha, u = 0
//         else:      beta = -sign(alpha) hypot(alpha, nu) (+hypot for alpha <= 0),
//                    t = (beta - alpha) / beta, u = a(j+1:, j) / (alpha - beta)
//       z_c = a(j,c) + (dot_c / M) (M / (alpha - beta)); rows i > j store u_i and
//       a(i,c) -= t u_i z_c; the owner of row j stores |beta| and d (a(j,c) - t z_c)
//       with d = +1 for beta >= 0 and -1 otherwise (R gets a non-negative
//       diagonal); thread 0 of workgroup 0 stores tau[j] = t and sig[j] = d.  From
//       the updated registers the workgroup writes its partials and the row copy
//       for column j + 1 under the other parity.  j = -1 only produces those.
//
// Nothing is squared or multiplied before it has been divided by a maximum, so
// the norm and the dots are safe wherever the stored values are: a matrix scaled
// by 2^+-600 (f64) factors like the unscaled one.  All sums run in double (f32
// included); u and t are rounded to the storage type before they are applied, so
// the stored reflector is the applied one.  The reference's rescue loop for
// |beta| < safeMin / epsilon (columns of subnormal size) is not implemented.
// A NaN or Inf propagates through max, norm and dots into the columns it reaches.
//
// Helpers of the block-reflector application (reflect/ApplyPacked/LLVF.hpp):
//   qr_explicit_u   U := the panel's reflectors, explicit: zero above the
//                   diagonal, 1 on it (no R entry is ever read as part of U);
//                   upper: the reflectors above the diagonal A(off + c, c)
//   qr_fix_t        T := tril(T) with diag(T) = 1 / t (FixDiagonal)
//   row_scale       A(i, :) *= sig[i0 + i * istride]
#include "kernels.hpp"
#include "dtype_switch.hpp"
#include "../common.hpp"
#include <climits>

namespace elx {
namespace kern {
namespace {

constexpr int R = kGeqrfLeafRows;
constexpr int W = kGeqrfLeafCols;
constexpr int NWAVE = R / 64;
constexpr int NACC = W + 1;  // sum of squares + W dots

// NaN-propagating max of non-negative values
__device__ __forceinline__ double nmax(double a, double b) { return (b > a || b != b) ? b : a; }

// the workgroup's max, in every thread
__device__ __forceinline__ double wg_max(double v, double* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = nmax(v, __shfl_xor(v, off));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();  // sh may still be read from an earlier call
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double b = sh[0];
#pragma unroll
    for (int q = 1; q < NWAVE; ++q) b = nmax(b, sh[q]);
    return b;
}

// the workgroup's sums of acc[0] and acc[lo..NACC), in every thread (the entries
// between are not needed and left alone); the same tree every time
__device__ __forceinline__ void wg_sum(double (&acc)[NACC], int lo, double* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NACC; ++c) {
        if (c != 0 && c < lo) continue;
        double v = acc[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) sh[wave * NACC + c] = v;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NACC; ++c) {
        if (c != 0 && c < lo) continue;
        double v = sh[c];
#pragma unroll
        for (int q = 1; q < NWAVE; ++q) v += sh[q * NACC + c];
        acc[c] = v;
    }
}

// scratch, by parity p: pm[p][np] maxima, pa[p][np][NACC] (sum of squares, then
// the dot with column c at 1 + c), rc[p][W] the copy of the pivot row
template <typename T>
__global__ __launch_bounds__(R) void geqrf_step_kernel(int j, int m, int w, int k, T* A, i64 lda, double* pm, double* pa,
                                                        double* rc, int np, T* tau, T* sig) {
    __shared__ double sh[NWAVE * NACC];
    const int tid = threadIdx.x;
    const int row = (int)blockIdx.x * R + tid;
    const bool in = row < m;
    T* arow = A + row;

    double a[W];
#pragma unroll
    for (int c = 0; c < W; ++c) a[c] = (in && c >= j && c < w) ? (double)arow[(i64)c * lda] : 0.0;

    if (j >= 0) {
        const int p = j & 1;
        const double* qm = pm + (size_t)p * np;
        const double* qa = pa + (size_t)p * np * NACC;
        const double* qr = rc + (size_t)p * W;
        // this thread's first partial and the pivot row, loaded before the first
        // barrier so that the launch waits for memory once
        double m0 = 0.0, p0[NACC], rj[W];
#pragma unroll
        for (int c = 0; c < NACC; ++c) p0[c] = 0.0;
        if (tid < np) {
            m0 = qm[tid];
            p0[0] = qa[(size_t)tid * NACC];
#pragma unroll
            for (int c = 1; c < W; ++c)
                if (c > j && c < w) p0[1 + c] = qa[(size_t)tid * NACC + 1 + c];
        }
#pragma unroll
        for (int c = 0; c < W; ++c) rj[c] = (c >= j && c < w) ? qr[c] : 0.0;
        double M = m0;
        for (int q = tid + R; q < np; q += R) M = nmax(M, qm[q]);
        M = wg_max(M, sh);
        double acc[NACC];
#pragma unroll
        for (int c = 0; c < NACC; ++c) acc[c] = 0.0;
        if (m0 != 0.0) {  // an all-zero part adds nothing; its sums are zero too
            const double r = m0 / M;
            acc[0] = p0[0] * r * r;
#pragma unroll
            for (int c = 1; c < W; ++c)
                if (c > j && c < w) acc[1 + c] = p0[1 + c] * r;
        }
        for (int q = tid + R; q < np; q += R) {
            const double mq = qm[q];
            if (mq == 0.0) continue;
            const double r = mq / M;
            acc[0] += qa[(size_t)q * NACC] * r * r;
#pragma unroll
            for (int c = 1; c < W; ++c)
                if (c > j && c < w) acc[1 + c] += qa[(size_t)q * NACC + 1 + c] * r;
        }
        wg_sum(acc, j + 2, sh);

        double alpha = 0.0;
#pragma unroll
        for (int c = 0; c < W; ++c)
            if (c == j) alpha = rj[c];
        double beta, t, d, scale;  // scale = M / (alpha - beta)
        const bool zero = M == 0.0;
        if (zero) {
            beta = -alpha;
            t = 2.0;
            scale = 0.0;
        } else {
            const double nu = M * sqrt(acc[0]);
            const double nrm = hypot(alpha, nu);
            beta = alpha <= 0.0 ? nrm : -nrm;
            t = (double)(T)((beta - alpha) / beta);
            scale = M / (alpha - beta);
        }
        d = beta >= 0.0 ? 1.0 : -1.0;
        const double denom = alpha - beta;

        if (in && row > j) {
            const T uT = zero ? T(0) : (T)(a[j] / denom);
            const double tu = t * (double)uT;
            arow[(i64)j * lda] = uT;
#pragma unroll
            for (int c = 1; c < W; ++c)
                if (c > j && c < w) {
                    const double z = rj[c] + acc[1 + c] * scale;
                    const T x = (T)(a[c] - tu * z);
                    arow[(i64)c * lda] = x;
                    a[c] = (double)x;
                }
        } else if (row == j) {
            arow[(i64)j * lda] = (T)(beta * d);
#pragma unroll
            for (int c = 1; c < W; ++c)
                if (c > j && c < w) {
                    const double z = rj[c] + acc[1 + c] * scale;
                    arow[(i64)c * lda] = (T)(d * (rj[c] - t * z));
                }
        }
        if (blockIdx.x == 0 && tid == 0) {
            tau[j] = (T)t;
            sig[j] = (T)d;
        }
    }

    const int jn = j + 1;
    if (jn >= k) return;  // uniform
    const int pn = jn & 1;
    // column jn over the rows below its diagonal
    double v = 0.0;
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (c == jn) v = a[c];
    const bool below = in && row > jn;
    if (!below) v = 0.0;
    const double mx = wg_max(fabs(v), sh);
    const double s = (below && mx != 0.0) ? v / mx : 0.0;
    double part[NACC];
#pragma unroll
    for (int c = 0; c < NACC; ++c) part[c] = 0.0;
    part[0] = s * s;
#pragma unroll
    for (int c = 1; c < W; ++c)
        if (c > jn && c < w) part[1 + c] = below ? s * a[c] : 0.0;
    wg_sum(part, jn + 2, sh);
    if (tid == 0) {
        pm[(size_t)pn * np + blockIdx.x] = mx;
        double* o = pa + ((size_t)pn * np + blockIdx.x) * NACC;
#pragma unroll
        for (int c = 0; c < NACC; ++c) o[c] = part[c];
    }
    if (in && row == jn) {
        double* o = rc + (size_t)pn * W;
#pragma unroll
        for (int c = 0; c < W; ++c)
            if (c >= jn && c < w) o[c] = a[c];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void qr_explicit_u_kernel(i64 m, i64 nb, const T* A, i64 lda, T* U, i64 ldu,
                                                            bool upper, i64 off) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const i64 c = blockIdx.y;
    if (i >= m || c >= nb) return;
    const i64 d = off + c;  // the row of the implicit 1
    const bool packed = upper ? i < d : i > d;
    U[i + c * ldu] = packed ? A[i + c * lda] : (i == d ? T(1) : T(0));
}

template <typename T>
__global__ __launch_bounds__(256) void qr_fix_t_kernel(i64 nb, T* S, i64 lds, const T* tau) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const i64 c = blockIdx.y;
    if (i > c || c >= nb) return;
    S[i + c * lds] = i == c ? T(1) / tau[c] : T(0);
}

template <typename T>
__global__ __launch_bounds__(256) void row_scale_kernel(i64 m, i64 n, T* A, i64 lda, const T* sig, i64 i0, i64 is) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const T d = sig[i0 + i * is];
    for (i64 c = blockIdx.y; c < n; c += gridDim.y) A[i + c * lda] *= d;
}

template <typename T>
hipError_t launch_leaf(i64 m, i64 w, T* A, i64 lda, T* tau, T* sig, void* work, hipStream_t s) {
    const int np = (int)((m + R - 1) / R);
    const int k = (int)std::min(m, w);
    double* pm = static_cast<double*>(work);
    double* pa = pm + 2 * (size_t)np;
    double* rc = pa + 2 * (size_t)np * NACC;
    for (int j = -1; j < k; ++j)
        hipLaunchKernelGGL((geqrf_step_kernel<T>), dim3(np), dim3(R), 0, s, j, (int)m, (int)w, k, A, lda, pm, pa, rc, np,
                           tau, sig);
    return hipGetLastError();
}

}  // namespace

size_t geqrf_work_bytes(i64 m) {
    const size_t np = (size_t)((m + R - 1) / R);
    return (2 * np * (1 + NACC) + 2 * W) * sizeof(double);
}

hipError_t geqrf_leaf(int dtype, i64 m, i64 w, void* A, i64 lda, void* tau, void* sig, void* work, hipStream_t s) {
    if (m <= 0 || w <= 0) return hipSuccess;
    if (w > W || m > INT_MAX - R || lda < m || !A || !tau || !sig || !work) return hipErrorInvalidValue;
    ELX_KERN_REAL_SWITCH(dtype, T,
                    return launch_leaf(m, w, static_cast<T*>(A), lda, static_cast<T*>(tau), static_cast<T*>(sig), work,
                                       s));
}

hipError_t qr_explicit_u(int dtype, i64 m, i64 nb, const void* A, i64 lda, void* U, i64 ldu, hipStream_t s, bool upper,
                         i64 off) {
    if (m <= 0 || nb <= 0) return hipSuccess;
    if (lda < m || ldu < m || nb > 65535 || m > (i64)256 * INT_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((m + 255) / 256), (unsigned)nb);
    ELX_KERN_REAL_SWITCH(dtype, T,
                    hipLaunchKernelGGL((qr_explicit_u_kernel<T>), grid, dim3(256), 0, s, m, nb,
                                       static_cast<const T*>(A), lda, static_cast<T*>(U), ldu, upper, off));
    return hipGetLastError();
}

hipError_t qr_fix_t(int dtype, i64 nb, void* S, i64 lds, const void* tau, hipStream_t s) {
    if (nb <= 0) return hipSuccess;
    if (lds < nb || nb > 65535 || !tau) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((nb + 255) / 256), (unsigned)nb);
    ELX_KERN_REAL_SWITCH(dtype, T,
                    hipLaunchKernelGGL((qr_fix_t_kernel<T>), grid, dim3(256), 0, s, nb, static_cast<T*>(S), lds,
                                       static_cast<const T*>(tau)));
    return hipGetLastError();
}

hipError_t row_scale(int dtype, i64 m, i64 n, void* A, i64 lda, const void* sig, i64 i0, i64 is, hipStream_t s) {
    if (m <= 0 || n <= 0) return hipSuccess;
    if (lda < m || !sig || m > (i64)256 * INT_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((m + 255) / 256), (unsigned)std::min<i64>(n, 1024));
    ELX_KERN_REAL_SWITCH(dtype, T,
                    hipLaunchKernelGGL((row_scale_kernel<T>), grid, dim3(256), 0, s, m, n, static_cast<T*>(A), lda,
                                       static_cast<const T*>(sig), i0, is));
    return hipGetLastError();
}

}  // namespace kern
}  // namespace elx
