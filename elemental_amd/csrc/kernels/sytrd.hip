// The panel of the blocked tridiagonalization (LAPACK's latrd form of
// herm_tridiag::LowerPanel / UpperPanel; the reference's sequential code is
// unblocked): w <= kSytrdMaxPanelCols columns of the n x n symmetric A are reduced,
// the reflectors V (explicit) and the vectors W of the deferred update
// A22 -= V W^T + W V^T are left in workspace, both n x w with leading dimension
// ldv and indexed by global row.
//
// Every kernel works on a ROW RANGE [r0, r1) of one column (a pointer to the
// column's row 0), one thread per row, kSytrdRows rows per workgroup; uplo lives
// in the caller's index arithmetic only:
//   lower, column c:  rows [c, n),     diagonal row rd = c, pivot row rp = c + 1
//   upper, column c:  rows [0, c + 1), diagonal row rd = c, pivot row rp = c - 1
// The tail of the reflector is the range without rd and rp; the ACTIVE range
// (the rows of v and w) is the range without rd.  As in geqrf.hip the global
// dependency is a kernel boundary: no grid barrier, no flags, no spinning, no
// floating-point atomics, nothing read back.  Per panel column j:
//
//   sytrd_refresh_kernel   finishes w_{j-1} := w' - (t/2)(w'.v) v from the dot
//       partials of the last step (W(:, j-1), rounded once), refreshes the column
//       a -= V(:, :j) W(rd, :j)^T + W(:, :j) V(rd, :j)^T, stores it, leaves per
//       workgroup the scaled norm pair (mx, sum (a/mx)^2) of the tail and the
//       pivot element alpha.  finish_only: the first part alone (after the last
//       column of a panel).
//   sytrd_reflect_kernel   combines the pairs in a fixed order into beta and t
//       (reflector::Col's convention, geqrf.hip), stores beta at the pivot row, u
//       in the tail, t, and v = [1; u] (0 at rd) into V(:, j); leaves per
//       workgroup the partials of V(:, :j)^T v and W(:, :j)^T v.
//   kern::symv             y := A22 v on the trailing triangle (two launches).
//   sytrd_w_kernel         w' := t (y - V (W^T v) - W (V^T v)) over the active
//       range, in double, with the partials of w'.v.
//
// Five launches per column, one more per panel.  Every workgroup adds partials in
// the same order, so two runs give the same bits.  Nothing is squared before it
// has been divided by the tail's maximum; sums run in double; u and t are rounded
// to the storage type before they are applied.  The rescue loop for subnormal
// columns is left out, as in geqrf.hip.  NaN and Inf propagate.
#include "kernels.hpp"
#include "dtype_switch.hpp"
#include "../common.hpp"
#include <climits>

namespace elx {
namespace kern {
namespace {

constexpr int R = kSytrdRows;
constexpr int WMAX = kSytrdMaxPanelCols;
constexpr int NWAVE = R / 64;
static_assert(R >= 2 * WMAX && R % 64 == 0, "one thread per panel partial");

// NaN-propagating max of non-negative values
__device__ __forceinline__ double nmax(double a, double b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the workgroup's max / sum, in every thread; the same tree every time
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
__device__ __forceinline__ double wg_sum(double v, double* sh) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double b = sh[0];
#pragma unroll
    for (int q = 1; q < NWAVE; ++q) b += sh[q];
    return b;
}

template <typename T>
__global__ __launch_bounds__(R) void sytrd_refresh_kernel(int r0, int r1, int rd, int rp, int j, bool finish_only,
                                                           T* col, const T* V, T* W, i64 ldv, const T* tprev,
                                                           const double* wp, const double* pd, int npd, double* pm,
                                                           double* pss, double* alpha_s) {
    __shared__ double sh[NWAVE], vrd[WMAX], wrd[WMAX];
    const int tid = threadIdx.x;
    const int row = r0 + (int)blockIdx.x * R + tid;
    const bool in = row < r1;

    // w_{j-1} = w' + coef v, coef = -(t/2) (w'.v): the dot's partials in index order
    double coef = 0.0;
    if (j > 0) {
        double d = 0.0;
        for (int q = 0; q < npd; ++q) d += pd[q];
        coef = -0.5 * (double)*tprev * d;
    }
    if (in && j > 0) W[row + (i64)(j - 1) * ldv] = (T)(wp[row] + coef * (double)V[row + (i64)(j - 1) * ldv]);
    if (finish_only) return;  // uniform

    // rows rd of V and W; W(rd, j-1) recomputed here, its owner may not have stored it yet
    if (tid < j) {
        const double v = (double)V[rd + (i64)tid * ldv];
        vrd[tid] = v;
        wrd[tid] = tid == j - 1 ? (double)(T)(wp[rd] + coef * v) : (double)W[rd + (i64)tid * ldv];
    }
    __syncthreads();
    double a = 0.0;
    if (in) {
        a = (double)col[row];
        for (int q = 0; q < j; ++q)
            a -= (double)V[row + (i64)q * ldv] * wrd[q] + (double)W[row + (i64)q * ldv] * vrd[q];
        const T ar = (T)a;
        col[row] = ar;
        a = (double)ar;
    }
    const bool tail = in && row != rd && row != rp;
    const double mx = wg_max(tail ? fabs(a) : 0.0, sh);
    const double sc = (tail && mx != 0.0) ? a / mx : 0.0;
    const double ss = wg_sum(sc * sc, sh);
    if (tid == 0) {
        pm[blockIdx.x] = mx;
        pss[blockIdx.x] = ss;
    }
    if (in && row == rp) *alpha_s = a;
}

template <typename T>
__global__ __launch_bounds__(R) void sytrd_reflect_kernel(int r0, int r1, int rd, int rp, int j, T* col, T* V,
                                                           const T* W, i64 ldv, T* tau, const double* pm,
                                                           const double* pss, int np, const double* alpha_s,
                                                           double* pv, double* pw) {
    __shared__ double sh[NWAVE], red[NWAVE][2 * WMAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = r0 + (int)blockIdx.x * R + tid;
    const bool in = row < r1;
    const double a = (in && row != rd) ? (double)col[row] : 0.0;
    const double alpha = *alpha_s;

    double M = 0.0;
    for (int q = tid; q < np; q += R) M = nmax(M, pm[q]);
    M = wg_max(M, sh);
    double acc = 0.0;
    for (int q = tid; q < np; q += R) {
        const double mq = pm[q];
        if (mq == 0.0) continue;  // an all-zero part adds nothing
        const double r = mq / M;
        acc += pss[q] * r * r;
    }
    acc = wg_sum(acc, sh);

    double beta, t, denom;
    const bool zero = M == 0.0;
    if (zero) {
        beta = -alpha;
        t = 2.0;
        denom = 1.0;
    } else {
        const double nrm = hypot(alpha, M * sqrt(acc));
        beta = alpha <= 0.0 ? nrm : -nrm;
        t = (double)(T)((beta - alpha) / beta);
        denom = alpha - beta;
    }
    double vi = 0.0;
    if (in) {
        T vT = T(0);
        if (row == rp) {
            col[row] = (T)beta;
            vT = T(1);
        } else if (row != rd) {
            vT = zero ? T(0) : (T)(a / denom);
            col[row] = vT;
        }
        V[row + (i64)j * ldv] = vT;
        vi = (double)vT;
    }
    if (blockIdx.x == 0 && tid == 0) *tau = (T)t;

    // this workgroup's part of V(:, :j)^T v and W(:, :j)^T v
    for (int q0 = 0; q0 < j; q0 += 8) {
        double sv[8], sw[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int q = q0 + u;
            const bool on = in && q < j;
            sv[u] = on ? (double)V[row + (i64)q * ldv] * vi : 0.0;
            sw[u] = on ? (double)W[row + (i64)q * ldv] * vi : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            sv[u] = wave_sum(sv[u]);
            sw[u] = wave_sum(sw[u]);
        }
        if (lane == 0) {
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (q0 + u < j) {
                    red[wave][q0 + u] = sv[u];
                    red[wave][WMAX + q0 + u] = sw[u];
                }
        }
    }
    __syncthreads();
    const int q = tid < WMAX ? tid : tid - WMAX;
    if (tid < 2 * WMAX && q < j) {
        const int slot = tid < WMAX ? q : WMAX + q;
        double s = red[0][slot];
#pragma unroll
        for (int k = 1; k < NWAVE; ++k) s += red[k][slot];
        (tid < WMAX ? pv : pw)[(size_t)blockIdx.x * WMAX + q] = s;
    }
}

template <typename T>
__global__ __launch_bounds__(R) void sytrd_w_kernel(int r0, int r1, int j, const T* V, const T* W, i64 ldv,
                                                     const T* tau, const T* y, const double* pv, const double* pw,
                                                     int np, double* wp, double* pd) {
    __shared__ double sh[NWAVE], g[2 * WMAX];  // g[q] = (V^T v)(q), g[WMAX + q] = (W^T v)(q)
    const int tid = threadIdx.x;
    const int row = r0 + (int)blockIdx.x * R + tid;
    const bool in = row < r1;
    const int q = tid < WMAX ? tid : tid - WMAX;
    if (tid < 2 * WMAX && q < j) {
        const double* p = tid < WMAX ? pv : pw;
        double s = 0.0;
        for (int b = 0; b < np; ++b) s += p[(size_t)b * WMAX + q];
        g[tid < WMAX ? q : WMAX + q] = s;
    }
    __syncthreads();
    double prod = 0.0;
    if (in) {
        double acc = (double)y[row];
        for (int c = 0; c < j; ++c)
            acc -= (double)V[row + (i64)c * ldv] * g[WMAX + c] + (double)W[row + (i64)c * ldv] * g[c];
        const double w = (double)*tau * acc;
        wp[row] = w;
        prod = w * (double)V[row + (i64)j * ldv];
    }
    prod = wg_sum(prod, sh);
    if (tid == 0) pd[blockIdx.x] = prod;
}

template <typename T>
hipError_t launch_panel(int dtype, bool lower, i64 n, i64 c0, i64 w, T* A, i64 lda, T* tau, T* V, T* W, i64 ldv, void* work,
                        hipStream_t s) {
    const size_t npm = (size_t)((n + R - 1) / R);
    double* pm = static_cast<double*>(work);
    double* pss = pm + npm;
    double* pd = pss + npm;
    double* alpha_s = pd + npm;
    double* pv = alpha_s + 1;
    double* pw = pv + npm * WMAX;
    double* wp = pw + npm * WMAX;
    T* y = reinterpret_cast<T*>(wp + n);
    auto blocks = [](int a, int b) { return (unsigned)((b - a + R - 1) / R); };
    int npd = 0;  // workgroups of the last sytrd_w_kernel
    const T* tprev = tau;
    int r0 = 0, r1 = 0;
    for (int j = 0; j < (int)w; ++j) {
        // column c, its range [r0, r1) and the active range [a0, a1)
        const int c = lower ? (int)c0 + j : (int)c0 - j;
        const int rd = c, rp = lower ? c + 1 : c - 1;
        r0 = lower ? c : 0;
        r1 = lower ? (int)n : c + 1;
        const int a0 = lower ? c + 1 : 0, a1 = lower ? (int)n : c;
        T* col = A + (i64)c * lda;
        T* tj = tau + (lower ? c : c - 1);
        const unsigned nb = blocks(r0, r1), nba = blocks(a0, a1);
        hipLaunchKernelGGL((sytrd_refresh_kernel<T>), dim3(nb), dim3(R), 0, s, r0, r1, rd, rp, j, false, col,
                           (const T*)V, W, ldv, tprev, (const double*)wp, (const double*)pd, npd, pm, pss, alpha_s);
        hipLaunchKernelGGL((sytrd_reflect_kernel<T>), dim3(nb), dim3(R), 0, s, r0, r1, rd, rp, j, col, V, (const T*)W,
                           ldv, tj, (const double*)pm, (const double*)pss, (int)nb, (const double*)alpha_s, pv, pw);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = symv(dtype, lower, a1 - a0, a1 - a0, 1.0, A + (i64)a0 * (lda + 1), lda, V + a0 + (i64)j * ldv, 1,
                 V + a0 + (i64)j * ldv, 1, 0.0, y + a0, 1, nullptr, 1, 0, 1, 0, 1, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((sytrd_w_kernel<T>), dim3(nba), dim3(R), 0, s, a0, a1, j, (const T*)V, (const T*)W, ldv,
                           (const T*)tj, (const T*)y, (const double*)pv, (const double*)pw, (int)nb, wp, pd);
        npd = (int)nba;
        tprev = tj;
        r0 = a0;
        r1 = a1;
    }
    // the last w of the panel, over its active range
    hipLaunchKernelGGL((sytrd_refresh_kernel<T>), dim3(blocks(r0, r1)), dim3(R), 0, s, r0, r1, 0, 0, (int)w, true,
                       (T*)nullptr, (const T*)V, W, ldv, tprev, (const double*)wp, (const double*)pd, npd, pm, pss,
                       alpha_s);
    return hipGetLastError();
}

}  // namespace

size_t sytrd_work_bytes(i64 n) {
    const size_t npm = (size_t)((n + R - 1) / R);
    // pm, pss, pd, alpha, pv, pw, w' (double) and y (at most 8 bytes an element)
    return (3 * npm + 1 + 2 * npm * WMAX + 2 * (size_t)n) * sizeof(double);
}

hipError_t sytrd_panel(int dtype, bool lower, i64 n, i64 c0, i64 w, void* A, i64 lda, void* tau, void* V, void* W,
                       i64 ldv, void* work, hipStream_t s) {
    if (n <= 1 || w <= 0) return hipSuccess;
    if (w > WMAX || n > INT_MAX - R || lda < n || ldv < n || !A || !tau || !V || !W || !work)
        return hipErrorInvalidValue;
    // the panel's columns: c0 .. c0 + w - 1 within [0, n - 2] (lower), c0 .. c0 - w + 1 within [1, n - 1] (upper)
    if (lower ? (c0 < 0 || c0 + w > n - 1) : (c0 > n - 1 || c0 - w < 0)) return hipErrorInvalidValue;
    ELX_KERN_REAL_SWITCH(dtype, T,
                         return launch_panel<T>(dtype, lower, n, c0, w, static_cast<T*>(A), lda, static_cast<T*>(tau),
                                             static_cast<T*>(V), static_cast<T*>(W), ldv, work, s));
}

}  // namespace kern
}  // namespace elx
