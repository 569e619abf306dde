// LU with partial pivoting of one tall column panel: the leaf of LocalLU
// (lu::Panel, src/lapack_like/factor/LU/Panel.hpp; the reference's GPU build hands
// the panel to the vendor solver).
//
// A leaf is m x w, w <= kGetrfLeafCols, column-major, m arbitrary (m >= w).  It
// does not fit one workgroup, and the pivot of column j depends on every row, so
// the leaf is spread over ceil(m / R) workgroups of R = kGetrfLeafRows threads,
// one thread per row, and the global dependency is a KERNEL BOUNDARY: one launch
// per column step.  No grid-wide barrier, no flags, no spinning.
//
// Pivoting is implicit inside the leaf: rows are not swapped while the steps run.
//   getrf_step_kernel(j)  every workgroup reduces the <= ceil(m / R) partial
//       (|value|, row) candidates of column j that the previous launch left (so
//       every workgroup knows the pivot row p_j without a second launch).  Row p_j
//       becomes "used": from here on nobody writes it, and it holds row j of U in
//       columns j.. and its multipliers in columns < j.  Every still-unused row i
//       computes l = a(i,j) / a(p_j,j), stores it in a(i,j) and updates
//       a(i, j+1..w-1) -= l a(p_j, j+1..w-1); the workgroup then writes its partial
//       candidate for column j + 1 over its unused rows.  The partials are
//       double-buffered by step parity (a launch reads parity j & 1 and writes the
//       other), so no workgroup writes what another reads in the same launch.
//       j = -1 only produces the partials of column 0.
//   getrf_finish_kernel   one workgroup turns p_0..p_{w-1} into the LAPACK swap
//       sequence (piv[j]: the row swapped with row j at step j, after the earlier
//       swaps), writes it to the device pivot array, and moves the <= 2w affected
//       rows of the leaf's own w columns to their final places through LDS (read
//       all, barrier, write), so overlapping sources and destinations are safe.
//   laswp_kernel          applies a run of swaps to a column range, pivots read
//       from device memory, one thread per column.
//
// Pivot rule: the largest |value|; ties go to the smallest row.  A NaN is turned
// into "no candidate" before it enters any reduction (candidate()), so it is never
// chosen, and never hides a number, while a number is left; a column
// whose unused entries are all zero or NaN counts as a zero pivot.  A zero pivot
// stores col0 + j + 1 into *info if that is still 0, and every launch that finds
// *info != 0 does nothing (the info-word contract of potrf_kernel).
#include "kernels.hpp"
#include "dtype_switch.hpp"
#include "../common.hpp"
#include <climits>

namespace elx {
namespace kern {
namespace {

constexpr int R = kGetrfLeafRows;
constexpr int W = kGetrfLeafCols;
constexpr int NWAVE = R / 64;

struct Cand {
    double v;  // |value|, -1: none
    int row;
};

__device__ __forceinline__ bool better(double v, int r, double bv, int br) {
    return v > bv || (v == bv && r < br);  // NaN v: false both ways
}

// A row's candidate.  A NaN becomes "none" HERE, before any reduction: `better`
// never displaces a NaN it already holds, so one that entered a reduction would
// hide the numbers reduced after it.
template <typename T>
__device__ __forceinline__ Cand candidate(T x, int row) {
    const double v = fabs((double)x);
    return v >= 0.0 ? Cand{v, row} : Cand{-1.0, INT_MAX};
}

// the best candidate of the workgroup, in every thread
__device__ __forceinline__ Cand wg_best(Cand c, Cand* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double v = __shfl_xor(c.v, off);
        const int r = __shfl_xor(c.row, off);
        if (better(v, r, c.v, c.row)) {
            c.v = v;
            c.row = r;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();  // sh may still be read from an earlier call
    if (lane == 0) sh[wave] = c;
    __syncthreads();
    Cand b = sh[0];
#pragma unroll
    for (int q = 1; q < NWAVE; ++q)
        if (better(sh[q].v, sh[q].row, b.v, b.row)) b = sh[q];
    return b;
}

// partials: pv[2][np] / pr[2][np] by step parity; prow[W]: the pivot rows so far
template <typename T>
__global__ __launch_bounds__(R) void getrf_step_kernel(int j, int m, int w, T* A, i64 lda, double* pv, int* pr,
                                                        int* prow, int np, int* info, int col0) {
    __shared__ Cand sh[NWAVE];
    __shared__ int failed;
    const int tid = threadIdx.x;
    if (tid == 0) failed = *info;
    __syncthreads();
    if (failed != 0) return;  // uniform: the whole workgroup leaves

    const int row = (int)blockIdx.x * R + tid;
    int p = -1;
    if (j >= 0) {
        Cand c{-1.0, INT_MAX};
        const double* v = pv + (size_t)(j & 1) * np;
        const int* r = pr + (size_t)(j & 1) * np;
        for (int q = tid; q < np; q += R)
            if (better(v[q], r[q], c.v, c.row)) c = Cand{v[q], r[q]};
        c = wg_best(c, sh);
        if (!(c.v > 0.0)) {  // an exact zero, or nothing but NaN: every workgroup sees the same
            if (blockIdx.x == 0 && tid == 0) *info = col0 + j + 1;
            return;
        }
        p = __builtin_amdgcn_readfirstlane(c.row);
        if (blockIdx.x == 0 && tid == 0) prow[j] = p;
    }

    bool live = row < m && row != p;
    for (int q = 0; q < j; ++q) live = live && prow[q] != row;  // rows used by earlier steps

    Cand mine{-1.0, INT_MAX};
    if (j < 0) {
        if (live) mine = candidate(A[row], row);
    } else {
        // row p_j of U first (nobody writes it in this launch), then this thread's row
        T u[W];
#pragma unroll
        for (int k = 0; k < W; ++k) u[k] = (k >= j && k < w) ? A[(i64)p + (i64)k * lda] : T(0);
        if (live) {
            T* a = A + row;
            T l = T(0), next = T(0);
#pragma unroll
            for (int k = 0; k < W; ++k) {
                if (k == j) {
                    l = a[(i64)k * lda] / u[k];
                    a[(i64)k * lda] = l;
                } else if (k > j && k < w) {
                    const T x = a[(i64)k * lda] - l * u[k];
                    a[(i64)k * lda] = x;
                    if (k == j + 1) next = x;
                }
            }
            mine = candidate(next, row);
        }
    }
    if (j + 1 < w) {
        const Cand b = wg_best(mine, sh);
        if (tid == 0) {
            pv[(size_t)((j + 1) & 1) * np + blockIdx.x] = b.v;
            pr[(size_t)((j + 1) & 1) * np + blockIdx.x] = b.row;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(R) void getrf_finish_kernel(int m, int w, T* A, i64 lda, const int* prow, int* piv,
                                                          int row_off, const int* info) {
    __shared__ int pos[2 * W], src[2 * W], count;
    __shared__ T rows[2 * W * W];
    if (*info != 0) return;  // nobody writes info here: uniform
    const int tid = threadIdx.x;
    if (tid == 0) {
        // the rows the swaps touch: positions 0..w-1 and the pivot rows beyond them;
        // src[k]: the original row that ends at position pos[k]
        int cnt = 0;
        for (int j = 0; j < w; ++j, ++cnt) pos[cnt] = src[cnt] = j;
        for (int j = 0; j < w; ++j) {
            const int p = prow[j];
            if (p >= w) {
                pos[cnt] = src[cnt] = p;
                ++cnt;
            }
        }
        for (int j = 0; j < w; ++j) {
            const int p = prow[j];
            int b = j;
            for (int q = 0; q < cnt; ++q)
                if (src[q] == p) b = q;  // p is unused before step j, so pos[b] >= j
            piv[j] = pos[b] + row_off;
            const int t = src[j];
            src[j] = src[b];
            src[b] = t;
        }
        count = cnt;
    }
    __syncthreads();
    const int total = count * w;
    for (int e = tid; e < total; e += R) {
        const int k = e / w, c = e - k * w;
        if (src[k] < m) rows[e] = A[(i64)src[k] + (i64)c * lda];
    }
    __syncthreads();
    for (int e = tid; e < total; e += R) {
        const int k = e / w, c = e - k * w;
        if (src[k] != pos[k] && src[k] < m && pos[k] < m) A[(i64)pos[k] + (i64)c * lda] = rows[e];
    }
}

// rows k and piv[k] - voff of columns [0, ncols) swapped for k = k0..k1-1 (inverse:
// in the opposite order); a pivot outside [0, m) is skipped
template <typename T>
__global__ __launch_bounds__(256) void laswp_kernel(i64 m, i64 ncols, T* A, i64 lda, const int* piv, i64 k0, i64 k1,
                                                     i64 voff, bool inverse, const int* info) {
    if (info && *info != 0) return;
    const i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncols) return;
    T* a = A + c * lda;
    for (i64 q = k0; q < k1; ++q) {
        const i64 k = inverse ? k0 + k1 - 1 - q : q;
        const i64 p = (i64)piv[k] - voff;
        if (p == k || p < 0 || p >= m || k >= m) continue;
        const T x = a[k];
        a[k] = a[p];
        a[p] = x;
    }
}

template <typename T>
hipError_t launch_leaf(i64 m, i64 w, T* A, i64 lda, int* piv, int row_off, void* work, int* info, int col0,
                       hipStream_t s) {
    const int np = (int)((m + R - 1) / R);
    double* pv = static_cast<double*>(work);
    int* pr = reinterpret_cast<int*>(pv + 2 * (size_t)np);
    int* prow = pr + 2 * (size_t)np;
    for (int j = -1; j < (int)w; ++j)
        hipLaunchKernelGGL((getrf_step_kernel<T>), dim3(np), dim3(R), 0, s, j, (int)m, (int)w, A, lda, pv, pr, prow, np,
                           info, col0);
    hipLaunchKernelGGL((getrf_finish_kernel<T>), dim3(1), dim3(R), 0, s, (int)m, (int)w, A, lda, prow, piv, row_off,
                       info);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_laswp(i64 m, i64 ncols, T* A, i64 lda, const int* piv, i64 k0, i64 k1, i64 voff, bool inverse,
                        const int* info, hipStream_t s) {
    hipLaunchKernelGGL((laswp_kernel<T>), dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, s, m, ncols, A, lda, piv,
                       k0, k1, voff, inverse, info);
    return hipGetLastError();
}

// ---- a run of swaps on the rows of a matrix distributed over `stride` process rows
// (global row P lives on process row (P + align) % stride as local row P / stride).
// Slot q < nbr stands for row k0 + q, slot nbr + q for row piv[k0 + q]: the 2 nbr
// rows the run can touch.  Every process row packs the slots it owns, the packed
// buffers are all-gathered down the process column, the swaps run on the gathered
// slots (redundantly, one thread per local column) and the owners unpack: the
// shapes depend on nbr and the grid alone, so the pivots stay on the device.
__device__ __forceinline__ i64 slot_row(const int* piv, i64 k0, i64 nbr, i64 q) {
    return q < nbr ? k0 + q : (i64)piv[k0 + q - nbr];
}

// meta[q]: the first slot that stands for the same row as slot q (-1: a row outside
// [0, m)); meta[2 nbr + q]: the process row that owns it
__global__ __launch_bounds__(256) void perm_meta_kernel(const int* piv, i64 k0, i64 nbr, i64 m, int stride, int align,
                                                         int* meta) {
    const i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= 2 * nbr) return;
    const i64 P = slot_row(piv, k0, nbr, q);
    i64 canon = q;
    if (P < 0 || P >= m) canon = -1;
    else if (q >= nbr) {
        if (P >= k0 && P < k0 + nbr) canon = P - k0;
        else
            for (i64 t = nbr; t < q; ++t)
                if ((i64)piv[k0 + t - nbr] == P) {
                    canon = t;
                    break;
                }
    }
    meta[q] = (int)canon;
    meta[2 * nbr + q] = P < 0 ? 0 : (int)((P + align) % stride);
}

// pack (scatter = false): buf(q, c) = A(local row of slot q, c) for the slots this
// process row owns; unpack (scatter = true): the reverse, from this rank's part
template <typename U>
__global__ __launch_bounds__(256) void perm_move_kernel(bool scatter, const int* piv, const int* meta, i64 k0, i64 nbr,
                                                         int stride, int rank, U* A, i64 lda, i64 lw, U* buf) {
    const i64 S = 2 * nbr;
    const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= S * lw) return;
    const i64 c = e / S, q = e - c * S;
    if (meta[q] != (int)q || meta[S + q] != rank) return;
    const i64 iloc = slot_row(piv, k0, nbr, q) / stride;
    if (scatter) A[iloc + c * lda] = buf[q + c * S];
    else buf[q + c * S] = A[iloc + c * lda];
}

// the swaps of the run on the gathered slots: slot q of column c lies in the part
// of its owner, g[(owner lw + c) S + q]
template <typename U>
__global__ __launch_bounds__(256) void perm_apply_kernel(const int* meta, i64 nbr, bool inverse, U* g, i64 lw) {
    const i64 S = 2 * nbr;
    const i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= lw) return;
    for (i64 t = 0; t < nbr; ++t) {
        const i64 k = inverse ? nbr - 1 - t : t;
        const int a = meta[k], b = meta[nbr + k];
        if (a < 0 || b < 0 || a == b) continue;
        U* pa = g + ((i64)meta[S + a] * lw + c) * S + a;
        U* pb = g + ((i64)meta[S + b] * lw + c) * S + b;
        const U x = *pa;
        *pa = *pb;
        *pb = x;
    }
}

}  // namespace

hipError_t perm_meta(const int* piv, i64 k0, i64 nbr, i64 m, int stride, int align, int* meta, hipStream_t s) {
    if (nbr <= 0) return hipSuccess;
    hipLaunchKernelGGL(perm_meta_kernel, dim3((unsigned)((2 * nbr + 255) / 256)), dim3(256), 0, s, piv, k0, nbr, m,
                       stride, align, meta);
    return hipGetLastError();
}

hipError_t perm_move(size_t elem_size, bool scatter, const int* piv, const int* meta, i64 k0, i64 nbr, int stride,
                     int rank, void* A, i64 lda, i64 lw, void* buf, hipStream_t s) {
    if (nbr <= 0 || lw <= 0) return hipSuccess;
    const i64 blocks = (2 * nbr * lw + 255) / 256;
    if (blocks > INT_MAX) return hipErrorInvalidValue;
    if (elem_size == 8)
        hipLaunchKernelGGL((perm_move_kernel<uint64_t>), dim3((unsigned)blocks), dim3(256), 0, s, scatter, piv, meta, k0,
                           nbr, stride, rank, static_cast<uint64_t*>(A), lda, lw, static_cast<uint64_t*>(buf));
    else if (elem_size == 4)
        hipLaunchKernelGGL((perm_move_kernel<uint32_t>), dim3((unsigned)blocks), dim3(256), 0, s, scatter, piv, meta, k0,
                           nbr, stride, rank, static_cast<uint32_t*>(A), lda, lw, static_cast<uint32_t*>(buf));
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t perm_apply(size_t elem_size, const int* meta, i64 nbr, bool inverse, void* gathered, i64 lw, hipStream_t s) {
    if (nbr <= 0 || lw <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((lw + 255) / 256);
    if (elem_size == 8)
        hipLaunchKernelGGL((perm_apply_kernel<uint64_t>), dim3(blocks), dim3(256), 0, s, meta, nbr, inverse,
                           static_cast<uint64_t*>(gathered), lw);
    else if (elem_size == 4)
        hipLaunchKernelGGL((perm_apply_kernel<uint32_t>), dim3(blocks), dim3(256), 0, s, meta, nbr, inverse,
                           static_cast<uint32_t*>(gathered), lw);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

size_t getrf_work_bytes(i64 m) {
    const size_t np = (size_t)((m + R - 1) / R);
    return 2 * np * sizeof(double) + 2 * np * sizeof(int) + W * sizeof(int);
}

hipError_t getrf_leaf(int dtype, i64 m, i64 w, void* A, i64 lda, int* piv, int row_off, void* work, int* info,
                      int col0, hipStream_t s) {
    if (m <= 0 || w <= 0) return hipSuccess;
    if (w > W || w > m || m > INT_MAX - R || lda < m || !piv || !work || !info) return hipErrorInvalidValue;
    ELX_KERN_REAL_SWITCH(dtype, T,
                    return launch_leaf(m, w, static_cast<T*>(A), lda, piv, row_off, work, info, col0, s));
}

hipError_t laswp(int dtype, i64 m, i64 ncols, void* A, i64 lda, const int* piv, i64 k0, i64 k1, i64 voff, bool inverse,
                 const int* info, hipStream_t s) {
    if (m <= 0 || ncols <= 0 || k1 <= k0) return hipSuccess;
    if (lda < m || !piv || k0 < 0 || ncols > (i64)256 * INT_MAX) return hipErrorInvalidValue;
    ELX_KERN_REAL_SWITCH(dtype, T,
                    return launch_laswp(m, ncols, static_cast<T*>(A), lda, piv, k0, k1, voff, inverse, info, s));
}

}  // namespace kern
}  // namespace elx
