// Device-side building blocks of the register-staged MFMA tile kernels
// (gemm_mfma.hip's gemm_tile_kernel, trmm.hip's trmm_tile_kernel): the
// 16x16x4 MFMA wrappers, the XCD-aware tile order, the LDS image of one
// operand k-slab and its loader, and the tile configurations.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace elx {
namespace kern {

using i64 = int64_t;

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <typename T> struct Mfma;
template <> struct Mfma<double> {
    using acc_t = f64x4;
    using pair_t = f64x2;
    static __device__ __forceinline__ acc_t op(double a, double b, acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    // C/D map of v_mfma_f64_16x16x4_f64: row = (lane>>4) + 4*reg, col = lane&15
    static __device__ __forceinline__ int row(int g, int r) { return g + 4 * r; }
};
template <> struct Mfma<float> {
    using acc_t = f32x4;
    using pair_t = f32x2;
    static __device__ __forceinline__ acc_t op(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    // C/D map of v_mfma_f32_16x16x4_f32: row = 4*(lane>>4) + reg, col = lane&15
    static __device__ __forceinline__ int row(int g, int r) { return 4 * g + r; }
};

constexpr int BK = 16, GROUP_M = 8;

// Map the flat workgroup id to a (tile_m, tile_n) pair.  Workgroups are dealt
// round-robin over the 8 XCDs (b and b+8 share one); remap so each XCD owns a
// contiguous run of the grouped order (bijective for any grid size).
__device__ __forceinline__ void tile_of(int bid, int nwg, int tiles_m, int tiles_n, int& tm, int& tn) {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    const int per_group = GROUP_M * tiles_n;
    const int group = wg / per_group;
    const int first_m = group * GROUP_M;
    const int gsz = min(tiles_m - first_m, GROUP_M);
    const int inner = wg - group * per_group;
    tm = first_m + inner % gsz;
    tn = inner / gsz;
}

// LDS image [k][r] of one operand slab (ROWS output rows x BK).
template <typename T, int ROWS, bool RCONTIG>
struct Img {
    static constexpr int P = RCONTIG ? ROWS + 16 : ROWS + 17;
    T d[BK][P];
    __device__ __forceinline__ T& at(int r, int k) { return d[k][r]; }
};

// Operand slab loader.  The operand is viewed as rows r (the output dimension:
// i for A, j for B) by k.  RCONTIG: X(r,k) = X[r + k*ld]; else X(r,k) = X[k + r*ld].
// Thread `tid` (of NTHR) owns element/pair p = tid + NTHR*q of the slab.
template <typename T, int ROWS, bool RCONTIG, bool VEC, int NTHR>
struct Slab {
    using pair_t = typename Mfma<T>::pair_t;
    static constexpr int STEP = VEC ? 2 : 1;
    static constexpr int EPT = ROWS * BK / NTHR;  // elements per thread
    static constexpr int NQ = EPT / STEP;          // loads per thread
    static __device__ __forceinline__ int r_of(int tid, int q) {
        const int p = tid + NTHR * q;
        if (RCONTIG) return VEC ? 2 * (p % (ROWS / 2)) : p % ROWS;
        return VEC ? p / (BK / 2) : p / BK;
    }
    static __device__ __forceinline__ int k_of(int tid, int q) {
        const int p = tid + NTHR * q;
        if (RCONTIG) return VEC ? p / (ROWS / 2) : p / ROWS;
        return VEC ? 2 * (p % (BK / 2)) : p % BK;
    }

    // Generic path (any alignment / size): 64-bit clamped addresses.
    static __device__ __forceinline__ void load_edge(const T* X, i64 ld, i64 rows, i64 kdim, i64 r0, i64 k0,
                                                     int tid, T (&v)[EPT], uint32_t& ok) {
        ok = 0;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const i64 r = r0 + r_of(tid, q), k = k0 + k_of(tid, q);
            ok |= (uint32_t)((r < rows) & (k < kdim)) << q;
            if (VEC) {  // pairs never straddle the edge: even extent along the vector dimension
                const i64 rc = r < rows ? r : rows - (RCONTIG ? 2 : 1);
                const i64 kc = k < kdim ? k : kdim - (RCONTIG ? 1 : 2);
                const pair_t x = *reinterpret_cast<const pair_t*>(RCONTIG ? X + rc + kc * ld : X + kc + rc * ld);
                v[2 * q] = x[0];
                v[2 * q + 1] = x[1];
            } else {
                const i64 rc = r < rows ? r : rows - 1, kc = k < kdim ? k : kdim - 1;
                v[q] = RCONTIG ? X[rc + kc * ld] : X[kc + rc * ld];
            }
        }
    }

    // 32-bit path (VEC, ld < 2^24): every load is one 32-bit offset off the
    // slab's uniform base; rows are clamped against the tile's uniform bound.
    struct Off32 {
        int rmax;  // last valid local row of this tile (uniform)
    };
    static __device__ __forceinline__ Off32 off32_init(int, i64 r0, i64 rows, uint32_t) {
        const i64 rm = rows - r0 - (RCONTIG && VEC ? 2 : 1);
        return Off32{rm > (1 << 30) ? (1 << 30) : (int)rm};
    }
    // sbase = X + slab origin (uniform); kleft = k extent left from the slab origin
    static __device__ __forceinline__ void load32(const T* sbase, const Off32& st, int tid, uint32_t ld, int kleft,
                                                  T (&v)[EPT], uint32_t& ok) {
        ok = 0;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int r = r_of(tid, q), kl = k_of(tid, q);
            const int rc = min(r, st.rmax);
            const int kc = min(kl, kleft - (RCONTIG ? 1 : 2));
            ok |= (uint32_t)((r <= st.rmax) & (kl < kleft)) << q;
            const uint32_t o = RCONTIG ? (uint32_t)rc + (uint32_t)kc * ld : (uint32_t)kc + (uint32_t)rc * ld;
            const pair_t x = *reinterpret_cast<const pair_t*>(sbase + o);
            v[2 * q] = x[0];
            v[2 * q + 1] = x[1];
        }
    }

    static __device__ __forceinline__ T sel(uint32_t ok, int q, T x) { return (ok >> q) & 1 ? x : T(0); }
    static __device__ __forceinline__ void store(Img<T, ROWS, RCONTIG>& S, int tid, const T (&v)[EPT], uint32_t ok) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int r = r_of(tid, q), k = k_of(tid, q);
            if (VEC) {
                S.at(r, k) = sel(ok, q, v[2 * q]);
                if (RCONTIG) S.at(r + 1, k) = sel(ok, q, v[2 * q + 1]);
                else S.at(r, k + 1) = sel(ok, q, v[2 * q + 1]);
            } else {
                S.at(r, k) = sel(ok, q, v[q]);
            }
        }
    }
};

template <int BM_, int BN_, int WAVES_M_, int WAVES_N_, int MINB_>
struct TileCfg {
    static constexpr int BM = BM_, BN = BN_, MINB = MINB_;
    static constexpr int WAVES_M = WAVES_M_, WAVES_N = WAVES_N_, NTHR = 64 * WAVES_M_ * WAVES_N_;
    static constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;  // wave tile
    static constexpr int WM = WTM / 16, WN = WTN / 16;            // MFMA tiles per wave
    static constexpr int WAVES_PER_EU = MINB_ * WAVES_M_ * WAVES_N_ / 4;
};
using Tile128 = TileCfg<128, 128, 2, 2, 2>;   // 4 waves of 64x64, 2 per SIMD
using Tile128w8 = TileCfg<128, 128, 4, 2, 2>; // 8 waves of 32x64, 4 per SIMD
using Tile256w8 = TileCfg<256, 128, 4, 2, 1>;  // 8 waves of 64x64, 2 per SIMD, 1 block/CU

}  // namespace kern
}  // namespace elx
