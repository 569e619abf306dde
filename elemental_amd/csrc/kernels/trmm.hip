// Triangular multiply for gfx950: C := alpha op(tri(A)) B, column-major, A m x m
// with only its uplo triangle read, B and C m x n (C apart from B).
//
// Replaces the reference's vendor call (LocalTrmm -> blas::Trmm ->
// rocblas_{s,d}trmm; src/blas_like/level3/Trmm.cpp:23-51, Trmm/LLN.hpp:178-228).
//
// gemm_mfma.hip's register-staged tile kernel with two changes:
//  * An output row tile [i0, i0+BM) walks only the k-slabs that meet op(A)'s
//    triangle in those rows (trmm_krange, kernels.hpp): half the MFMA work of
//    the full product.  Row tiles have unequal k lengths: the tile order
//    (trmm_tile_of) gives every XCD all of them, the long ones first.
//  * op(A) goes through registers into LDS, and the triangle is a select at
//    that LDS store: an element outside the triangle becomes 0 and a unit
//    diagonal 1 whatever memory holds there (NaN, Inf), never a product with
//    zero.  Only slabs that straddle the diagonal (BM/BK per tile) take the
//    masked store, by a slab-uniform branch; the rest store as the GEMM does.
// Static LDS: f64 128x64 tiles (8 waves of 32x32, two workgroups per CU,
// 56.5 KiB), f32 256x128 tiles (8 waves of 64x64, 52.3 KiB).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels.hpp"
#include "dtype_switch.hpp"
#include "../common.hpp"
#include "mfma_tile.hpp"

namespace elx {
namespace kern {

template <typename T> struct TrmmTile;
template <> struct TrmmTile<double> { using type = TileCfg<kTrmmBM64, 64, 4, 2, 2>; };  // 8 waves of 32x32, 4 per SIMD
template <> struct TrmmTile<float> { using type = TileCfg<kTrmmBM32, 128, 4, 2, 1>; };  // 8 waves of 64x64, 2 per SIMD
static_assert(kTrmmBK == BK, "trmm_krange's slab is the tile kernels' BK");

template <typename T>
struct TrmmParams {
    i64 m, n;
    T alpha;
    const T* A; i64 lda;
    const T* B; i64 ldb;
    T* C; i64 ldc;
    int tiles_m, tiles_n;
    bool unit;
};

// LDS store of an op(A) slab that straddles the diagonal.  d0 = (tile's first
// row) - (slab's first k): element (r, k) of the slab lies d = r + d0 - k below
// the diagonal.  L: op(A) is lower, d > 0 is stored; else d < 0.
template <typename T, typename SA, int ROWS, bool RCONTIG, bool VEC, bool L>
__device__ __forceinline__ void store_tri(Img<T, ROWS, RCONTIG>& S, int tid, const T (&v)[SA::EPT], uint32_t ok,
                                          int d0, bool unit) {
    auto pick = [&](uint32_t in, int d, T x) {
        const T diag = unit ? T(1) : x;
        const T t = (L ? d > 0 : d < 0) ? x : (d == 0 ? diag : T(0));
        return in ? t : T(0);
    };
#pragma unroll
    for (int q = 0; q < SA::NQ; ++q) {
        const int r = SA::r_of(tid, q), k = SA::k_of(tid, q);
        const uint32_t in = (ok >> q) & 1;
        const int d = r + d0 - k;
        if (VEC) {
            S.at(r, k) = pick(in, d, v[2 * q]);
            if (RCONTIG) S.at(r + 1, k) = pick(in, d + 1, v[2 * q + 1]);
            else S.at(r, k + 1) = pick(in, d - 1, v[2 * q + 1]);
        } else {
            S.at(r, k) = pick(in, d, v[q]);
        }
    }
}

// Map the flat workgroup id to (tm, tn), tm ranked by k length (0 = longest).
// As tile_of, each XCD owns a contiguous run of the order, but row tiles have
// unequal k ranges, so a run must hold every row tile or one XCD gets all the
// long ones: the order goes by blocks of tiles_n/8 column tiles (one per XCD),
// and inside a block by groups of GROUP_M adjacent row tiles, longest first.
// The workgroups resident on an XCD are then a group's row tiles (k ranges
// within GROUP_M tiles of each other, so they walk k together and share the
// slabs in L2) over a few of the block's columns.  Bijective for any grid.
__device__ __forceinline__ void trmm_tile_of(int bid, int nwg, int tiles_m, int tiles_n, int& tm, int& tn) {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    const int cbw = (tiles_n + 7) >> 3;  // column tiles per block
    const int blk = wg / (cbw * tiles_m);
    const int c0 = blk * cbw, cw = min(cbw, tiles_n - c0);
    const int rem = wg - blk * cbw * tiles_m;
    const int per_group = GROUP_M * cw;
    const int group = rem / per_group;
    const int first_m = group * GROUP_M;
    const int gsz = min(tiles_m - first_m, GROUP_M);
    const int inner = rem - group * per_group;
    tm = first_m + inner % gsz;
    tn = c0 + inner / gsz;
}

// TA: op(A) = A^T.  L: op(A) is lower (lower != TA).  FAST: 16-byte loads off
// 32-bit offsets (aligned bases, even m / lda / ldb, lda and ldb < 2^24).
template <typename T, typename CFG, bool TA, bool L, bool FAST>
__global__ __launch_bounds__(CFG::NTHR, CFG::WAVES_PER_EU) void trmm_tile_kernel(TrmmParams<T> p) {
    using M = Mfma<T>;
    using acc_t = typename M::acc_t;
    constexpr int BM = CFG::BM, BN = CFG::BN, WM = CFG::WM, WN = CFG::WN;
    constexpr int WTM = CFG::WTM, WTN = CFG::WTN;
    constexpr bool RA = !TA;  // op(A)(i,k): !TA -> A[i + k*lda]; B(k,j) = B[k + j*ldb]
    using SA = Slab<T, BM, RA, FAST, CFG::NTHR>;
    using SB = Slab<T, BN, false, FAST, CFG::NTHR>;
    __shared__ __attribute__((aligned(16))) Img<T, BM, RA> As[2];
    __shared__ __attribute__((aligned(16))) Img<T, BN, false> Bs[2];
    static_assert(sizeof(As) + sizeof(Bs) <= 64 * 1024, "static LDS");

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave / CFG::WAVES_N, wc = wave % CFG::WAVES_N;
    const int g = lane >> 4, c = lane & 15;

    int tm, tn;
    trmm_tile_of(blockIdx.x, gridDim.x, p.tiles_m, p.tiles_n, tm, tn);
    if (L) tm = p.tiles_m - 1 - tm;  // op(A) lower: the last row tile has the longest k range
    const i64 m0 = (i64)tm * BM, n0 = (i64)tn * BN;
    const TrmmKRange kr = trmm_krange(L, p.m, m0, BM);
    const i64 kend = kr.k1;  // B's rows and op(A)'s columns at or beyond kend are never touched

    acc_t acc[WM][WN];
#pragma unroll
    for (int a = 0; a < WM; ++a)
#pragma unroll
        for (int b = 0; b < WN; ++b) acc[a][b] = acc_t{0, 0, 0, 0};

    const int kt0 = (int)(kr.k0 / BK), kt1 = (int)((kend + BK - 1) / BK);
    typename SA::Off32 sta{};
    typename SB::Off32 stb{};
    if (FAST) {
        sta = SA::off32_init(tid, m0, p.m, (uint32_t)p.lda);
        stb = SB::off32_init(tid, n0, p.n, (uint32_t)p.ldb);
    }
    T ra[SA::EPT], rb[SB::EPT];
    uint32_t oka = 0, okb = 0;
    auto load_slab = [&](int kt) {
        const i64 k0 = (i64)kt * BK;
        if (FAST) {
            const i64 kl = kend - k0;
            const int kleft = kl > (1 << 20) ? (1 << 20) : (int)kl;
            SA::load32(p.A + (RA ? m0 + k0 * p.lda : m0 * p.lda + k0), sta, tid, (uint32_t)p.lda, kleft, ra, oka);
            SB::load32(p.B + (n0 * p.ldb + k0), stb, tid, (uint32_t)p.ldb, kleft, rb, okb);
        } else {
            SA::load_edge(p.A, p.lda, p.m, kend, m0, k0, tid, ra, oka);
            SB::load_edge(p.B, p.ldb, p.n, kend, n0, k0, tid, rb, okb);
        }
    };
    auto store_slab = [&](int kt, int buf) {
        const i64 k0 = (i64)kt * BK;
        // wholly inside the triangle (slab-uniform): the GEMM's store
        const bool inside = L ? k0 + BK <= m0 : k0 >= m0 + BM;
        if (inside) SA::store(As[buf], tid, ra, oka);
        else store_tri<T, SA, BM, RA, FAST, L>(As[buf], tid, ra, oka, (int)(m0 - k0), p.unit);
        SB::store(Bs[buf], tid, rb, okb);
    };
    load_slab(kt0);  // kt0 < kt1: every row tile meets the diagonal
    store_slab(kt0, 0);
    __syncthreads();

    for (int kt = kt0; kt < kt1; ++kt) {
        const int cur = (kt - kt0) & 1;
        const bool more = (kt + 1) < kt1;
        if (more) load_slab(kt + 1);  // issued early; lands during the MFMAs
#pragma unroll
        for (int s = 0; s < BK / 4; ++s) {
            T a[WM], b[WN];
#pragma unroll
            for (int mi = 0; mi < WM; ++mi) a[mi] = As[cur].at(wr * WTM + mi * 16 + c, 4 * s + g);
#pragma unroll
            for (int ni = 0; ni < WN; ++ni) b[ni] = Bs[cur].at(wc * WTN + ni * 16 + c, 4 * s + g);
#pragma unroll
            for (int mi = 0; mi < WM; ++mi)
#pragma unroll
                for (int ni = 0; ni < WN; ++ni) acc[mi][ni] = M::op(a[mi], b[ni], acc[mi][ni]);
        }
        if (more) store_slab(kt + 1, cur ^ 1);
        __syncthreads();
    }

    const i64 ib = m0 + wr * WTM, jb = n0 + wc * WTN;
    const bool interior = ib + WTM <= p.m && jb + WTN <= p.n;
#pragma unroll
    for (int mi = 0; mi < WM; ++mi) {
#pragma unroll
        for (int ni = 0; ni < WN; ++ni) {
            const i64 j = jb + ni * 16 + c;
            if (!interior && j >= p.n) continue;
            T* ccol = p.C + j * p.ldc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const i64 i = ib + mi * 16 + M::row(g, r);
                if (interior || i < p.m) ccol[i] = p.alpha * acc[mi][ni][r];
            }
        }
    }
}

template <typename T, typename CFG, bool TA, bool L>
static hipError_t launch_trmm(TrmmParams<T> p, hipStream_t s) {
    p.tiles_m = (int)((p.m + CFG::BM - 1) / CFG::BM);
    p.tiles_n = (int)((p.n + CFG::BN - 1) / CFG::BN);
    const i64 nwg = (i64)p.tiles_m * p.tiles_n;
    if (nwg > 0x7fffffff) return hipErrorInvalidValue;
    // 16-byte loads need 16-byte aligned bases, even leading dimensions and an
    // even m (A's and B's unit-stride extents; every k range then ends even)
    auto al = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    const bool fast = al(p.A) && al(p.B) && p.lda % 2 == 0 && p.ldb % 2 == 0 && p.m % 2 == 0 &&
                      p.lda < (1 << 24) && p.ldb < (1 << 24);
    if (fast)
        hipLaunchKernelGGL((trmm_tile_kernel<T, CFG, TA, L, true>), dim3((unsigned)nwg), dim3(CFG::NTHR), 0, s, p);
    else
        hipLaunchKernelGGL((trmm_tile_kernel<T, CFG, TA, L, false>), dim3((unsigned)nwg), dim3(CFG::NTHR), 0, s, p);
    return hipGetLastError();
}

template <typename T>
static hipError_t trmm_typed(bool lower, bool trans, bool unit, i64 m, i64 n, double alpha, const void* A, i64 lda,
                             const void* B, i64 ldb, void* C, i64 ldc, hipStream_t s) {
    using CFG = typename TrmmTile<T>::type;
    const TrmmParams<T> p{m, n, (T)alpha, static_cast<const T*>(A), lda, static_cast<const T*>(B), ldb,
                          static_cast<T*>(C), ldc, 0, 0, unit};
    if (trans) return lower ? launch_trmm<T, CFG, true, false>(p, s) : launch_trmm<T, CFG, true, true>(p, s);
    return lower ? launch_trmm<T, CFG, false, true>(p, s) : launch_trmm<T, CFG, false, false>(p, s);
}

hipError_t trmm_tri(int dtype, bool lower, bool trans, bool unit, i64 m, i64 n, double alpha, const void* A, i64 lda,
                    const void* B, i64 ldb, void* C, i64 ldc, hipStream_t s) {
    if (m <= 0 || n <= 0) return hipSuccess;
    if (lda < m || ldb < m || ldc < m) return hipErrorInvalidValue;
    ELX_KERN_REAL_SWITCH(dtype, T,
                    return trmm_typed<T>(lower, trans, unit, m, n, alpha, A, lda, B, ldb, C, ldc, s));
}

}  // namespace kern
}  // namespace elx
