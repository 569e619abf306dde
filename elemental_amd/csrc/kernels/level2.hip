// Level-2 BLAS kernels (gfx950): Gemv, Symv, Ger, Syr, Syr2.  All of them are
// bound by HBM: each reads (or reads and writes) every matrix element it needs
// exactly once, 16 bytes per lane where the base and the leading dimension allow
// it and element by element otherwise.
//
// Matrices are column-major with any lda; vectors have an element stride.  Sums
// are kept in double for f64 and in float for f32 / f16 / bf16 and rounded to the
// storage type once.  No floating-point atomics: where the sum of one output
// element is split over workgroups, each workgroup writes its partial to pool
// workspace and level2_reduce_kernel adds the partials in index order, so two
// calls on the same input give the same bits.
//
// Thread layout shared by gemv_n, symv and the rank updates: a tile of ROWS rows
// is walked by RL = ROWS / VEC row-lanes of VEC = 16 B / sizeof(element)
// consecutive rows each (a wave reads 1 KiB of one column at a time), and the
// NT / RL column groups take the tile's columns round-robin.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "dtype_switch.hpp"
#include <algorithm>

namespace elx {
namespace kern {

namespace {

constexpr int NT = 256;

template <typename S>
struct alignas(16) Vec16 {
    S v[16 / sizeof(S)];
};

template <typename T, int ROWS>
struct Lay {
    using S = typename Elem<T>::storage;
    static constexpr int VEC = 16 / (int)sizeof(S);
    static constexpr int RL = ROWS / VEC;
    static constexpr int CG = NT / RL;
    static_assert(ROWS % VEC == 0 && NT % RL == 0 && RL <= NT, "tile does not fit the workgroup");
};

// rows [0, nvalid) of the VEC rows at p, the rest zero; one 16-B load when allowed
template <typename T, int VEC>
__device__ __forceinline__ void load_rows(const typename Elem<T>::storage* p, bool vec, i64 nvalid,
                                          typename Elem<T>::compute (&a)[VEC]) {
    using S = typename Elem<T>::storage;
    if (vec && nvalid >= VEC) {
        const Vec16<S> v = *reinterpret_cast<const Vec16<S>*>(p);
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] = Elem<T>::load(v.v[e]);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] = e < nvalid ? Elem<T>::load(p[e]) : typename Elem<T>::compute(0);
    }
}

template <typename T>
__device__ __forceinline__ void finish(typename Elem<T>::storage* y, typename Elem<T>::compute alpha,
                                       typename Elem<T>::compute acc, typename Elem<T>::compute beta) {
    using C = typename Elem<T>::compute;
    // beta == 0: y is output only (a NaN there does not survive)
    const C v = beta == C(0) ? alpha * acc : alpha * acc + beta * Elem<T>::load(*y);
    *y = Elem<T>::store(v);
}

// y := alpha A x + beta y (part null) or part[split][i] := (A x)(i) over the
// split's columns.  grid (ceil(m / kGemvRows), splits)
template <typename T>
__global__ __launch_bounds__(NT) void gemv_n_kernel(i64 m, i64 n, typename Elem<T>::compute alpha,
                                                    const typename Elem<T>::storage* A, i64 lda,
                                                    const typename Elem<T>::storage* x, i64 incx,
                                                    typename Elem<T>::compute beta, typename Elem<T>::storage* y,
                                                    i64 incy, typename Elem<T>::compute* part, i64 cols_per_split,
                                                    bool vec) {
    using E = Elem<T>;
    using C = typename E::compute;
    using L = Lay<T, kGemvRows>;
    constexpr int VEC = L::VEC, RL = L::RL, CG = L::CG;
    static_assert(kGemvCols <= NT, "one x element per thread and chunk");
    __shared__ C xs[kGemvCols];
    __shared__ C red[CG > 1 ? (CG - 1) * kGemvRows : 1];
    const int tid = threadIdx.x, rl = tid % RL, cg = tid / RL;
    const i64 r0 = (i64)blockIdx.x * kGemvRows + (i64)rl * VEC;
    const i64 nvalid = m - r0 < VEC ? m - r0 : VEC;  // <= 0: no rows here
    const i64 jbeg = (i64)blockIdx.y * cols_per_split;
    const i64 jend = jbeg + cols_per_split < n ? jbeg + cols_per_split : n;
    C acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = C(0);
    for (i64 jc = jbeg; jc < jend; jc += kGemvCols) {
        const int w = (int)(jend - jc < kGemvCols ? jend - jc : kGemvCols);
        __syncthreads();
        if (tid < w) xs[tid] = E::load(x[(jc + tid) * incx]);
        __syncthreads();
        if (nvalid <= 0) continue;
        const typename E::storage* a = A + r0 + jc * lda;
        int c = cg;
        for (; c + 3 * CG < w; c += 4 * CG) {
            C v[4][VEC];
#pragma unroll
            for (int u = 0; u < 4; ++u) load_rows<T, VEC>(a + (i64)(c + u * CG) * lda, vec, nvalid, v[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const C xv = xs[c + u * CG];
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] += v[u][e] * xv;
            }
        }
        for (; c < w; c += CG) {
            C v[VEC];
            load_rows<T, VEC>(a + (i64)c * lda, vec, nvalid, v);
            const C xv = xs[c];
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] += v[e] * xv;
        }
    }
    if (CG > 1) {
        if (cg > 0) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) red[(cg - 1) * kGemvRows + rl * VEC + e] = acc[e];
        }
        __syncthreads();
        if (cg == 0) {
            for (int g = 1; g < CG; ++g) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] += red[(g - 1) * kGemvRows + rl * VEC + e];
            }
        }
    }
    if (cg != 0) return;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        if (e >= nvalid) break;
        const i64 i = r0 + e;
        if (part) part[(i64)blockIdx.y * m + i] = acc[e];
        else finish<T>(y + i * incy, alpha, acc[e], beta);
    }
}

// y := alpha A^T x + beta y (part null) or part[split][j] := (A^T x)(j) over the
// split's rows: one wave per column, lanes stride down the rows.
// grid (ceil(n / kGemvTCols), splits)
template <typename T>
__global__ __launch_bounds__(NT) void gemv_t_kernel(i64 m, i64 n, typename Elem<T>::compute alpha,
                                                    const typename Elem<T>::storage* A, i64 lda,
                                                    const typename Elem<T>::storage* x, i64 incx,
                                                    typename Elem<T>::compute beta, typename Elem<T>::storage* y,
                                                    i64 incy, typename Elem<T>::compute* part, i64 rows_per_split,
                                                    bool vec, bool xvec) {
    using E = Elem<T>;
    using C = typename E::compute;
    using S = typename E::storage;
    constexpr int VEC = 16 / (int)sizeof(S);
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const i64 j = (i64)blockIdx.x * kGemvTCols + wave;
    const i64 ibeg = (i64)blockIdx.y * rows_per_split;
    const i64 iend = ibeg + rows_per_split < m ? ibeg + rows_per_split : m;
    C acc = C(0);
    if (j < n) {
        const S* a = A + j * lda;
#pragma unroll 4
        for (i64 i = ibeg + (i64)lane * VEC; i < iend; i += 64 * VEC) {
            const i64 nvalid = iend - i < VEC ? iend - i : VEC;
            C av[VEC], xv[VEC];
            load_rows<T, VEC>(a + i, vec, nvalid, av);
            if (xvec && nvalid >= VEC) {
                load_rows<T, VEC>(x + i, true, nvalid, xv);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) xv[e] = e < nvalid ? E::load(x[(i + e) * incx]) : C(0);
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc += av[e] * xv[e];
        }
    }
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane != 0 || j >= n) return;
    if (part) part[(i64)blockIdx.y * n + j] = acc;
    else finish<T>(y + j * incy, alpha, acc, beta);
}

// The global index map of a local block: local (i, j) is global (i0 + i is, j0 +
// j js); lower: the triangle gi >= gj, else gi <= gj.
struct TriMap {
    int lower;
    i64 m, n, i0, is, j0, js;
};
__host__ __device__ __forceinline__ bool tri_in(const TriMap& p, i64 i, i64 j) {
    const i64 gi = p.i0 + i * p.is, gj = p.j0 + j * p.js;
    return p.lower ? gi >= gj : gi <= gj;
}
__host__ __device__ __forceinline__ bool tri_strict(const TriMap& p, i64 i, i64 j) {
    const i64 gi = p.i0 + i * p.is, gj = p.j0 + j * p.js;
    return p.lower ? gi > gj : gi < gj;
}
// rows [r0, r1) x columns [c0, c1) of the local block: 0 nothing of it lies in
// the triangle, 2 all of it strictly inside, 1 anything else (masked by index)
__host__ __device__ __forceinline__ int tri_class(const TriMap& p, i64 r0, i64 r1, i64 c0, i64 c1) {
    const i64 gi0 = p.i0 + r0 * p.is, gi1 = p.i0 + (r1 - 1) * p.is;
    const i64 gj0 = p.j0 + c0 * p.js, gj1 = p.j0 + (c1 - 1) * p.js;
    if (p.lower) return gi0 > gj1 ? 2 : gi1 < gj0 ? 0 : 1;
    return gi1 < gj0 ? 2 : gi0 > gj1 ? 0 : 1;
}
__host__ __device__ __forceinline__ bool symv_tile_live(const TriMap& p, i64 ti, i64 tj) {
    const i64 r0 = ti * kSymvTile, c0 = tj * kSymvTile;
    const i64 r1 = r0 + kSymvTile < p.m ? r0 + kSymvTile : p.m, c1 = c0 + kSymvTile < p.n ? c0 + kSymvTile : p.n;
    return r0 < r1 && c0 < c1 && tri_class(p, r0, r1, c0, c1) != 0;
}

// One kSymvTile^2 tile of the triangle per workgroup, each element read once and
// used twice from registers:
//   prow[tj][i] := sum_{j in tile, (i,j) in the triangle} a(i,j) xc[j]
//   pcol[ti][j] := sum_{i in tile, (i,j) strictly inside} a(i,j) xr[i]
// Tiles outside the triangle return at once and leave their slots unwritten
// (level2_reduce_kernel skips them by the same test).  grid (row tiles, column tiles)
template <typename T>
__global__ __launch_bounds__(NT) void symv_kernel(TriMap mp, const typename Elem<T>::storage* A, i64 lda,
                                                  const typename Elem<T>::storage* xr, i64 incxr,
                                                  const typename Elem<T>::storage* xc, i64 incxc,
                                                  typename Elem<T>::compute* prow, typename Elem<T>::compute* pcol,
                                                  bool vec) {
    using E = Elem<T>;
    using C = typename E::compute;
    using L = Lay<T, kSymvTile>;
    constexpr int TS = kSymvTile, VEC = L::VEC, RL = L::RL, CG = L::CG, CPT = TS / CG;
    static_assert(RL <= 64 && 64 % RL == 0 && CPT % 4 == 0 && CG > 1, "symv layout");
    const i64 ti = blockIdx.x, tj = blockIdx.y;
    const i64 r0 = ti * TS, c0 = tj * TS;
    const i64 r1 = r0 + TS < mp.m ? r0 + TS : mp.m, c1 = c0 + TS < mp.n ? c0 + TS : mp.n;
    const int cls = tri_class(mp, r0, r1, c0, c1);
    if (cls == 0) return;
    __shared__ C xcs[TS], zcs[TS], red[(CG - 1) * TS];
    const int tid = threadIdx.x, rl = tid % RL, cg = tid / RL;
    if (tid < TS) xcs[tid] = c0 + tid < c1 ? E::load(xc[(c0 + tid) * incxc]) : C(0);
    const i64 i = r0 + (i64)rl * VEC;
    const i64 nvalid = r1 - i < VEC ? r1 - i : VEC;
    C xrv[VEC], zr[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        xrv[e] = e < nvalid ? E::load(xr[(i + e) * incxr]) : C(0);
        zr[e] = C(0);
    }
    __syncthreads();
    for (int k = 0; k < CPT; k += 4) {
        C a[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const i64 j = c0 + cg + (k + u) * CG;
#pragma unroll
            for (int e = 0; e < VEC; ++e) a[u][e] = C(0);
            if (j >= c1 || nvalid <= 0) continue;
            if (cls == 2) {
                load_rows<T, VEC>(A + i + j * lda, vec, nvalid, a[u]);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    if (e < nvalid && tri_in(mp, i + e, j)) a[u][e] = E::load(A[i + e + j * lda]);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = cg + (k + u) * CG;
            const i64 j = c0 + c;
            const C xv = xcs[c];
            C zc = C(0);
            if (cls == 2) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    zr[e] += a[u][e] * xv;
                    zc += a[u][e] * xrv[e];
                }
            } else if (j < c1) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (e < nvalid && tri_in(mp, i + e, j)) zr[e] += a[u][e] * xv;
                    if (e < nvalid && tri_strict(mp, i + e, j)) zc += a[u][e] * xrv[e];
                }
            }
            for (int off = RL / 2; off >= 1; off >>= 1) zc += __shfl_down(zc, off, RL);
            if (rl == 0) zcs[c] = zc;
        }
    }
    if (cg > 0) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) red[(cg - 1) * TS + rl * VEC + e] = zr[e];
    }
    __syncthreads();
    if (cg == 0) {
        for (int g = 1; g < CG; ++g) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) zr[e] += red[(g - 1) * TS + rl * VEC + e];
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            if (e < nvalid) prow[tj * mp.m + i + e] = zr[e];
    }
    if (tid < TS && c0 + tid < c1) pcol[ti * mp.n + c0 + tid] = zcs[tid];
}

// y(i) := alpha (sum_s p1[s][i] + sum_s p2[s][i]) + beta y(i), the partials added
// in index order.  symv: p1 are symv_kernel's row partials (slot = column tile),
// p2 its column partials (slot = row tile); only live tiles' slots are read.
// No partials at all: y := beta y.
template <typename T>
__global__ __launch_bounds__(NT) void level2_reduce_kernel(i64 len, typename Elem<T>::compute alpha,
                                                           const typename Elem<T>::compute* p1, int ns1,
                                                           const typename Elem<T>::compute* p2, int ns2,
                                                           typename Elem<T>::compute beta,
                                                           typename Elem<T>::storage* y, i64 incy, bool symv,
                                                           TriMap mp) {
    using C = typename Elem<T>::compute;
    const i64 i = (i64)blockIdx.x * NT + threadIdx.x;
    if (i >= len) return;
    C acc = C(0);
    for (int s = 0; s < ns1; ++s)
        if (!symv || symv_tile_live(mp, i / kSymvTile, s)) acc += p1[(i64)s * len + i];
    for (int s = 0; s < ns2; ++s)
        if (!symv || symv_tile_live(mp, s, i / kSymvTile)) acc += p2[(i64)s * len + i];
    if (ns1 + ns2 == 0) {
        y[i * incy] = beta == C(0) ? Elem<T>::store(C(0)) : Elem<T>::store(beta * Elem<T>::load(y[i * incy]));
        return;
    }
    finish<T>(y + i * incy, alpha, acc, beta);
}

// A(i,j) += alpha (xr[i] yc[j] [+ yr[i] xc[j]]) on the whole block (MODE 0, Ger),
// or on the triangle of the index map with one (MODE 1, Syr) or two (MODE 2,
// Syr2) terms; the other triangle is neither read nor written.
// grid (ceil(m / kGerRows), ceil(n / kGerCols))
template <typename T, int MODE>
__device__ __forceinline__ void rank_update(const TriMap& mp, typename Elem<T>::compute alpha,
                                            const typename Elem<T>::storage* xr, i64 incxr,
                                            const typename Elem<T>::storage* yc, i64 incyc,
                                            const typename Elem<T>::storage* yr, i64 incyr,
                                            const typename Elem<T>::storage* xc, i64 incxc,
                                            typename Elem<T>::storage* A, i64 lda, bool vec) {
    using E = Elem<T>;
    using C = typename E::compute;
    using S = typename E::storage;
    using L = Lay<T, kGerRows>;
    constexpr int VEC = L::VEC, RL = L::RL, CG = L::CG;
    static_assert(kGerCols <= NT && kGerCols % CG == 0, "rank-update layout");
    const i64 r0 = (i64)blockIdx.x * kGerRows, c0 = (i64)blockIdx.y * kGerCols;
    const i64 r1 = r0 + kGerRows < mp.m ? r0 + kGerRows : mp.m, c1 = c0 + kGerCols < mp.n ? c0 + kGerCols : mp.n;
    const int cls = MODE == 0 ? 2 : tri_class(mp, r0, r1, c0, c1);
    if (cls == 0) return;
    __shared__ C cs[kGerCols], ct[MODE == 2 ? kGerCols : 1];
    const int tid = threadIdx.x, rl = tid % RL, cg = tid / RL;
    if (tid < kGerCols && c0 + tid < c1) {
        cs[tid] = E::load(yc[(c0 + tid) * incyc]);
        if (MODE == 2) ct[tid] = E::load(xc[(c0 + tid) * incxc]);
    }
    __syncthreads();
    const i64 i = r0 + (i64)rl * VEC;
    const i64 nvalid = r1 - i < VEC ? r1 - i : VEC;
    if (nvalid <= 0) return;
    C u[VEC], v[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        u[e] = e < nvalid ? alpha * E::load(xr[(i + e) * incxr]) : C(0);
        v[e] = MODE == 2 && e < nvalid ? alpha * E::load(yr[(i + e) * incyr]) : C(0);
    }
    const bool whole = cls == 2 && vec && nvalid >= VEC;
#pragma unroll 4
    for (int c = cg; c < (int)(c1 - c0); c += CG) {
        S* a = A + i + (c0 + c) * lda;
        const C sv = cs[c], tv = MODE == 2 ? ct[c] : C(0);
        if (whole) {
            Vec16<S> w = *reinterpret_cast<const Vec16<S>*>(a);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                C z = E::load(w.v[e]) + u[e] * sv;
                if (MODE == 2) z += v[e] * tv;
                w.v[e] = E::store(z);
            }
            *reinterpret_cast<Vec16<S>*>(a) = w;
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                if (e >= nvalid || (cls != 2 && !tri_in(mp, i + e, c0 + c))) continue;
                C z = E::load(a[e]) + u[e] * sv;
                if (MODE == 2) z += v[e] * tv;
                a[e] = E::store(z);
            }
        }
    }
}

#define ELX_RANK_ARGS                                                                                        \
    TriMap mp, typename Elem<T>::compute alpha, const typename Elem<T>::storage *xr, i64 incxr,              \
        const typename Elem<T>::storage *yc, i64 incyc, const typename Elem<T>::storage *yr, i64 incyr,     \
        const typename Elem<T>::storage *xc, i64 incxc, typename Elem<T>::storage *A, i64 lda, bool vec
template <typename T>
__global__ __launch_bounds__(NT) void ger_kernel(ELX_RANK_ARGS) {
    rank_update<T, 0>(mp, alpha, xr, incxr, yc, incyc, yr, incyr, xc, incxc, A, lda, vec);
}
template <typename T>
__global__ __launch_bounds__(NT) void syr_kernel(ELX_RANK_ARGS) {
    rank_update<T, 1>(mp, alpha, xr, incxr, yc, incyc, yr, incyr, xc, incxc, A, lda, vec);
}
template <typename T>
__global__ __launch_bounds__(NT) void syr2_kernel(ELX_RANK_ARGS) {
    rank_update<T, 2>(mp, alpha, xr, incxr, yc, incyc, yr, incyr, xc, incxc, A, lda, vec);
}
#undef ELX_RANK_ARGS

bool Aligned16(const void* p, i64 ld, size_t es) {
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && (ld * (i64)es) % 16 == 0;
}

template <typename T>
hipError_t gemv_t(bool trans, i64 m, i64 n, double alpha, const void* A_, i64 lda, const void* x_, i64 incx,
                  double beta, void* y_, i64 incy, hipStream_t s) {
    using S = typename Elem<T>::storage;
    using C = typename Elem<T>::compute;
    const S* A = static_cast<const S*>(A_);
    const S* x = static_cast<const S*>(x_);
    S* y = static_cast<S*>(y_);
    const Level2Plan pl = gemv_plan(trans, m, n);
    const i64 ylen = trans ? n : m;
    const bool vec = Aligned16(A, lda, sizeof(S));
    C* part = nullptr;
    if (pl.splits > 1) {
        const hipError_t e = workspace_alloc(reinterpret_cast<void**>(&part), sizeof(C) * (size_t)pl.splits * ylen, s);
        if (e != hipSuccess) return e;
    }
    if (!trans) {
        const dim3 grid((unsigned)((m + kGemvRows - 1) / kGemvRows), (unsigned)pl.splits);
        hipLaunchKernelGGL((gemv_n_kernel<T>), grid, dim3(NT), 0, s, m, n, (C)alpha, A, lda, x, incx, (C)beta, y, incy,
                           part, pl.per, vec);
    } else {
        const bool xvec = incx == 1 && reinterpret_cast<uintptr_t>(x) % 16 == 0;
        const dim3 grid((unsigned)((n + kGemvTCols - 1) / kGemvTCols), (unsigned)pl.splits);
        hipLaunchKernelGGL((gemv_t_kernel<T>), grid, dim3(NT), 0, s, m, n, (C)alpha, A, lda, x, incx, (C)beta, y, incy,
                           part, pl.per, vec, xvec);
    }
    hipError_t e = hipGetLastError();
    if (part) {
        if (e == hipSuccess) {
            hipLaunchKernelGGL((level2_reduce_kernel<T>), dim3((unsigned)((ylen + NT - 1) / NT)), dim3(NT), 0, s, ylen,
                               (C)alpha, part, pl.splits, (const C*)nullptr, 0, (C)beta, y, incy, false, TriMap{});
            e = hipGetLastError();
        }
        const hipError_t f = workspace_free(part, s);
        if (e == hipSuccess) e = f;
    }
    return e;
}

template <typename T>
void launch_reduce(i64 len, double alpha, const typename Elem<T>::compute* p1, int ns1,
                   const typename Elem<T>::compute* p2, int ns2, double beta, void* y, i64 incy, bool symv,
                   const TriMap& mp, hipStream_t s) {
    using C = typename Elem<T>::compute;
    hipLaunchKernelGGL((level2_reduce_kernel<T>), dim3((unsigned)((len + NT - 1) / NT)), dim3(NT), 0, s, len, (C)alpha,
                       p1, ns1, p2, ns2, (C)beta, static_cast<typename Elem<T>::storage*>(y), incy, symv, mp);
}

}  // namespace

Level2Plan gemv_plan(bool trans, i64 m, i64 n) {
    // the dimension the sum runs over, in chunks; the other one gives the workgroups
    const i64 chunk = trans ? kGemvRows : kGemvCols;
    const i64 k = trans ? m : n;
    const i64 wgs = trans ? (n + kGemvTCols - 1) / kGemvTCols : (m + kGemvRows - 1) / kGemvRows;
    const i64 chunks = (k + chunk - 1) / chunk;
    Level2Plan pl{1, std::max<i64>(chunks, 1) * chunk};
    // fewer workgroups than CUs: split the sum for two workgroups per CU
    if (wgs <= 0 || wgs >= 256 || chunks < 2) return pl;
    i64 z = std::min<i64>(std::min<i64>(chunks, (512 + wgs - 1) / wgs), kLevel2MaxSplits);
    const i64 per = (chunks + z - 1) / z;
    z = (chunks + per - 1) / per;
    if (z < 2) return pl;
    pl.splits = (int)z;
    pl.per = per * chunk;
    return pl;
}

hipError_t gemv(int dtype, bool trans, i64 m, i64 n, double alpha, const void* A, i64 lda, const void* x, i64 incx,
                double beta, void* y, i64 incy, hipStream_t s) {
    const i64 ylen = trans ? n : m, xlen = trans ? m : n;
    if (ylen <= 0) return hipSuccess;
    if (xlen <= 0 || alpha == 0.0) return vec_scale(dtype, ylen, beta, y, incy, s);
    if ((m + kGemvRows - 1) / kGemvRows > 0x7fffffffll || (n + kGemvTCols - 1) / kGemvTCols > 0x7fffffffll)
        return hipErrorInvalidValue;
    ELX_KERN_SWITCH(dtype, T, return gemv_t<T>(trans, m, n, alpha, A, lda, x, incx, beta, y, incy, s));
    return hipSuccess;
}

hipError_t vec_scale(int dtype, i64 len, double beta, void* y, i64 incy, hipStream_t s) {
    if (len <= 0 || beta == 1.0) return hipSuccess;
    ELX_KERN_SWITCH(dtype, T, launch_reduce<T>(len, 0.0, nullptr, 0, nullptr, 0, beta, y, incy, false, TriMap{}, s));
    return hipGetLastError();
}

hipError_t symv(int dtype, bool lower, i64 m, i64 n, double alpha, const void* A, i64 lda, const void* xr, i64 incxr,
                const void* xc, i64 incxc, double beta, void* zr, i64 inczr, void* zc, i64 inczc, i64 i0, i64 is,
                i64 j0, i64 js, hipStream_t s) {
    if (m <= 0 || n <= 0 || alpha == 0.0) {
        hipError_t e = vec_scale(dtype, m, beta, zr, inczr, s);
        if (e == hipSuccess && zc) e = vec_scale(dtype, n, beta, zc, inczc, s);
        return e;
    }
    if (is < 1 || js < 1 || (!zc && m != n)) return hipErrorInvalidValue;
    const i64 nti = (m + kSymvTile - 1) / kSymvTile, ntj = (n + kSymvTile - 1) / kSymvTile;
    if (ntj > 65535 || nti > 0x7fffffffll) return hipErrorInvalidValue;
    const TriMap mp{lower ? 1 : 0, m, n, i0, is, j0, js};
    ELX_KERN_REAL_SWITCH(dtype, T, {
        using S = typename Elem<T>::storage;
        using C = typename Elem<T>::compute;
        C* part = nullptr;
        hipError_t e = workspace_alloc(reinterpret_cast<void**>(&part), sizeof(C) * (size_t)(ntj * m + nti * n), s);
        if (e != hipSuccess) return e;
        C* prow = part;
        C* pcol = part + ntj * m;
        hipLaunchKernelGGL((symv_kernel<T>), dim3((unsigned)nti, (unsigned)ntj), dim3(NT), 0, s, mp,
                           static_cast<const S*>(A), lda, static_cast<const S*>(xr), incxr, static_cast<const S*>(xc),
                           incxc, prow, pcol, Aligned16(A, lda, sizeof(S)));
        e = hipGetLastError();
        if (e == hipSuccess) {
            if (zc) {
                launch_reduce<T>(m, alpha, prow, (int)ntj, nullptr, 0, beta, zr, inczr, true, mp, s);
                launch_reduce<T>(n, alpha, nullptr, 0, pcol, (int)nti, beta, zc, inczc, true, mp, s);
            } else {
                launch_reduce<T>(m, alpha, prow, (int)ntj, pcol, (int)nti, beta, zr, inczr, true, mp, s);
            }
            e = hipGetLastError();
        }
        const hipError_t f = workspace_free(part, s);
        return e == hipSuccess ? f : e;
    });
    return hipSuccess;
}

hipError_t rank_update(int dtype, int terms, bool lower, i64 m, i64 n, double alpha, const void* xr, i64 incxr,
                       const void* yc, i64 incyc, const void* yr, i64 incyr, const void* xc, i64 incxc, void* A,
                       i64 lda, i64 i0, i64 is, i64 j0, i64 js, hipStream_t s) {
    if (m <= 0 || n <= 0 || alpha == 0.0) return hipSuccess;
    if (terms < 0 || terms > 2 || is < 1 || js < 1) return hipErrorInvalidValue;
    const i64 gx = (m + kGerRows - 1) / kGerRows;
    if (gx > 0x7fffffffll) return hipErrorInvalidValue;
    ELX_KERN_REAL_SWITCH(dtype, T, {
        using S = typename Elem<T>::storage;
        using C = typename Elem<T>::compute;
        const bool vec = Aligned16(A, lda, sizeof(S));
        // column blocks of at most 65535 workgroups each
        const i64 cmax = 65535ll * kGerCols;
        for (i64 c0 = 0; c0 < n; c0 += cmax) {
            const i64 nc = std::min<i64>(cmax, n - c0);
            const TriMap mp{lower ? 1 : 0, m, nc, i0, is, j0 + c0 * js, js};
            const dim3 grid((unsigned)gx, (unsigned)((nc + kGerCols - 1) / kGerCols));
            const S* ycp = static_cast<const S*>(yc) + c0 * incyc;
            const S* xcp = terms == 2 ? static_cast<const S*>(xc) + c0 * incxc : nullptr;
            S* a = static_cast<S*>(A) + c0 * lda;
            auto* kernel = terms == 0 ? ger_kernel<T> : terms == 1 ? syr_kernel<T> : syr2_kernel<T>;
            hipLaunchKernelGGL(kernel, grid, dim3(NT), 0, s, mp, (C)alpha, static_cast<const S*>(xr), incxr, ycp,
                               incyc, static_cast<const S*>(yr), incyr, xcp, incxc, a, lda, vec);
        }
    });
    return hipGetLastError();
}

}  // namespace kern
}  // namespace elx
