// The two diagonal-block leaves of El::TriangularInverse and El::Trtrmm
// (triang_inv::LVar3Unb / UVar3Unb, Triangular/LVar3.hpp:17-43, and
// trtrmm::LUnblocked / UUnblocked, Trtrmm/Unblocked.hpp:16-115, on A11[*,*]).
//
// One workgroup of NW waves holds the n x n block (n <= kTrtriMax) in LDS and
// works on it in place.  The uplo triangle is staged as the LOWER triangle of S
// exactly as potrf.hip stages it: padded to np = a multiple of 16 with an
// identity, zero above the diagonal, and for UPPER transposed at the load and
// again at the store.  Both operations commute with that transpose
// ((U^T)^-1 = (U^-1)^T, U U^T = S^T S with S = U^T) and with the padding
// (blockdiag(L, I) goes to blockdiag(L^-1, I) and blockdiag(L^T L, I)), so the
// kernels know the lower case only and no loop has an edge.  Nothing outside
// the n x n triangle is stored, and with a unit diagonal the diagonal is
// neither loaded nor stored.
//
// trtri_kernel   S := S^-1.
//   1. the np/16 diagonal 16 x 16 blocks, one per wave: lane c (< 16) solves
//      D x = e_c by forward substitution in registers, D read from LDS as
//      wave-wide broadcasts; column c goes back after a barrier.
//   2. levels h = 16, 32, 64: every aligned 2h block [L11 0; L21 L22] has X11 and
//      X22 in place and gets X21 = -X22 (L21 X11) in two MFMA passes over
//      16 x 16 tiles: T = L21 X11 is held in accumulators, written over L21
//      after a barrier, and X21 = -X22 T is formed and written the same way.  At
//      most 16 tiles per pass (h = 64, np = 128): two accumulators per wave and
//      no scratch beside S.  Four barriers per level.
//   No singularity test: an exact zero on a NON_UNIT diagonal divides and
//   leaves Inf / NaN, as the reference's loop does.
//
// lauum_kernel   S := S^T S on the lower triangle.
//   R(I,J) = sum_{K >= I} S(K,I)^T S(K,J) for the 16 x 16 tiles I >= J: at most
//   36 tiles, dealt round-robin, five accumulators per wave.  Every tile is
//   formed in registers from the old S, one barrier, then all are written.
#include "kernels.hpp"
#include "dtype_switch.hpp"
#include "mfma_tile.hpp"
#include "../common.hpp"

namespace elx {
namespace kern {
namespace {

constexpr int PW = 16;  // MFMA tile
constexpr int NW = 8;   // waves per workgroup
constexpr int NTHR = 64 * NW;
constexpr int kMaxTiles = (int)(kTrtriMax / PW);                          // 8
constexpr int kTrtriAcc = (kMaxTiles / 2) * (kMaxTiles / 2) / NW;         // 2: the h = 64 pass
constexpr int kLauumAcc = (kMaxTiles * (kMaxTiles + 1) / 2 + NW - 1) / NW;  // 5

__host__ __device__ constexpr i64 trtri_np(i64 n) { return (n + PW - 1) / PW * PW; }
__host__ __device__ constexpr i64 trtri_ld(i64 np) { return np + 1; }
template <typename T>
constexpr size_t trtri_lds(i64 n) {
    return (size_t)trtri_np(n) * trtri_ld(trtri_np(n)) * sizeof(T);
}

// S(i,j) = the triangle for n > i >= j (the diagonal only when !unit), identity
// in the padding and on a unit diagonal, 0 above
template <typename T>
__device__ __forceinline__ void stage_lower(T* S, int np, int ld, bool lower, bool unit, int n, const T* A, i64 lda) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < np; c += NW) {
        for (int r = lane; r < np; r += 64) {
            // LOWER: c is the column, r the row (unit stride in A and in S);
            // UPPER: S(c, r) = A[r + c*lda], r <= c
            const int i = lower ? r : c, j = lower ? c : r;
            T v = i == j ? T(1) : T(0);
            if (i < n && (unit ? i > j : i >= j)) v = A[(i64)r + (i64)c * lda];
            S[i + j * ld] = v;
        }
    }
}

template <typename T>
__device__ __forceinline__ void store_lower(const T* S, int ld, bool lower, bool unit, int n, T* A, i64 lda) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < n; c += NW) {
        for (int r = lane; r < n; r += 64) {
            const int i = lower ? r : c, j = lower ? c : r;
            if (unit ? i > j : i >= j) A[(i64)r + (i64)c * lda] = S[i + j * ld];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(NTHR) void trtri_kernel(bool lower, bool unit, int n, T* A, i64 lda) {
    using M = Mfma<T>;
    using acc_t = typename M::acc_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int np = (int)trtri_np(n), ld = (int)trtri_ld(np), nt = np / PW;
    T* S = reinterpret_cast<T*>(smem);
    auto at = [&](int i, int j) -> T& { return S[i + j * ld]; };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c16 = lane & 15;

    stage_lower(S, np, ld, lower, unit, n, A, lda);
    __syncthreads();

    // ---- 1. the diagonal blocks: wave w owns block w; lane c its column c
    const int p0 = wave * PW;
    T x[PW];
    if (wave < nt) {
#pragma unroll
        for (int i = 0; i < PW; ++i) {
            T acc = i == c16 ? T(1) : T(0);
#pragma unroll
            for (int k = 0; k < i; ++k) acc -= at(p0 + i, p0 + k) * x[k];  // x[k] = 0 for k < c16
            x[i] = acc / at(p0 + i, p0 + i);
        }
    }
    __syncthreads();  // D is read; X goes over it
    if (wave < nt && lane < PW) {
#pragma unroll
        for (int i = 0; i < PW; ++i)
            if (i >= c16) at(p0 + i, p0 + c16) = x[i];
    }
    __syncthreads();

    // ---- 2. the blocks under the diagonal, level by level
    for (int h = PW; h < np; h *= 2) {
        const int kt = h / PW;                   // tiles per side of L11 / L22
        const int npairs = (np + 2 * h - 1) / (2 * h);
        const int ntile = npairs * kt * kt;      // <= kTrtriAcc * NW
        // pass 0: T = L21 X11; pass 1: X21 = -X22 T
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            acc_t acc[kTrtriAcc];
#pragma unroll
            for (int q = 0; q < kTrtriAcc; ++q) {
                const int t = wave + NW * q;
                const int pair = t / (kt * kt), I = (t / kt) % kt, J = t % kt;
                const int r0 = pair * 2 * h, mid = r0 + h;
                acc[q] = acc_t{0, 0, 0, 0};
                if (t >= ntile || mid + I * PW >= np) continue;  // wave-uniform
                const int K0 = pass == 0 ? J : 0, K1 = pass == 0 ? kt : I + 1;
                for (int K = K0; K < K1; ++K) {
#pragma unroll
                    for (int s = 0; s < PW / 4; ++s) {
                        const int k = K * PW + 4 * s + g;
                        T a, b;
                        if (pass == 0) {
                            a = at(mid + I * PW + c16, r0 + k);   // L21(I,K)
                            b = at(r0 + k, r0 + J * PW + c16);    // X11(K,J)
                        } else {
                            a = -at(mid + I * PW + c16, mid + k);  // X22(I,K)
                            b = at(mid + k, r0 + J * PW + c16);    // T(K,J)
                        }
                        acc[q] = M::op(a, b, acc[q]);
                    }
                }
            }
            __syncthreads();  // every read of the old L21 (pass 0) / T (pass 1) is done
#pragma unroll
            for (int q = 0; q < kTrtriAcc; ++q) {
                const int t = wave + NW * q;
                const int pair = t / (kt * kt), I = (t / kt) % kt, J = t % kt;
                const int r0 = pair * 2 * h, mid = r0 + h;
                if (t >= ntile || mid + I * PW >= np) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) at(mid + I * PW + M::row(g, r), r0 + J * PW + c16) = acc[q][r];
            }
            __syncthreads();
        }
    }

    store_lower(S, ld, lower, unit, n, A, lda);
}

template <typename T>
__global__ __launch_bounds__(NTHR) void lauum_kernel(bool lower, int n, T* A, i64 lda) {
    using M = Mfma<T>;
    using acc_t = typename M::acc_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int np = (int)trtri_np(n), ld = (int)trtri_ld(np), nt = np / PW;
    T* S = reinterpret_cast<T*>(smem);
    auto at = [&](int i, int j) -> T& { return S[i + j * ld]; };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c16 = lane & 15;

    stage_lower(S, np, ld, lower, false, n, A, lda);
    __syncthreads();

    // tile t of the packed lower triangle: I(I+1)/2 + J, J <= I
    const int ntile = nt * (nt + 1) / 2;
    auto tile_of = [&](int t, int& I, int& J) {
        I = 0;
        while ((I + 1) * (I + 2) / 2 <= t) ++I;
        J = t - I * (I + 1) / 2;
    };
    acc_t acc[kLauumAcc];
#pragma unroll
    for (int q = 0; q < kLauumAcc; ++q) {
        const int t = wave + NW * q;
        acc[q] = acc_t{0, 0, 0, 0};
        if (t >= ntile) continue;  // wave-uniform
        int I, J;
        tile_of(t, I, J);
        for (int K = I; K < nt; ++K) {
#pragma unroll
            for (int s = 0; s < PW / 4; ++s) {
                const int k = K * PW + 4 * s + g;
                const T a = at(k, I * PW + c16);  // S(K,I)^T
                const T b = at(k, J * PW + c16);  // S(K,J)
                acc[q] = M::op(a, b, acc[q]);
            }
        }
    }
    __syncthreads();  // every read of the old S is done
#pragma unroll
    for (int q = 0; q < kLauumAcc; ++q) {
        const int t = wave + NW * q;
        if (t >= ntile) continue;
        int I, J;
        tile_of(t, I, J);
        // a diagonal tile is written whole (it is symmetric); only i >= j is stored
#pragma unroll
        for (int r = 0; r < 4; ++r) at(I * PW + M::row(g, r), J * PW + c16) = acc[q][r];
    }
    __syncthreads();

    store_lower(S, ld, lower, false, n, A, lda);
}

template <typename T>
hipError_t raise_lds_limit(const void* kernel) {
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)trtri_lds<T>(kTrtriMax));
}

template <typename T>
hipError_t launch_trtri(bool lower, bool unit, i64 n, T* A, i64 lda, hipStream_t s) {
    const size_t lds = trtri_lds<T>(n);
    if (lds > 64 * 1024) {  // beyond the default dynamic-LDS limit (gfx950: 160 KiB per workgroup)
        static const hipError_t e = raise_lds_limit<T>(reinterpret_cast<const void*>(&trtri_kernel<T>));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((trtri_kernel<T>), dim3(1), dim3(NTHR), lds, s, lower, unit, (int)n, A, lda);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_lauum(bool lower, i64 n, T* A, i64 lda, hipStream_t s) {
    const size_t lds = trtri_lds<T>(n);
    if (lds > 64 * 1024) {
        static const hipError_t e = raise_lds_limit<T>(reinterpret_cast<const void*>(&lauum_kernel<T>));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((lauum_kernel<T>), dim3(1), dim3(NTHR), lds, s, lower, (int)n, A, lda);
    return hipGetLastError();
}

static_assert(kTrtriMax == kPotrfMax, "the three leaves share one block size");
static_assert(kTrtriMax % PW == 0 && kTrtriAcc * NW >= (kMaxTiles / 2) * (kMaxTiles / 2),
              "trtri: the widest level must fit the accumulators");
static_assert(trtri_lds<double>(kTrtriMax) <= 160 * 1024, "kTrtriMax: the f64 block must fit one workgroup's LDS");

}  // namespace

hipError_t trtri_block(int dtype, bool lower, bool unit, i64 n, void* A, i64 lda, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (n > kTrtriMax || lda < n) return hipErrorInvalidValue;
    ELX_KERN_REAL_SWITCH(dtype, T,
                    return launch_trtri(lower, unit, n, static_cast<T*>(A), lda, s));
}

hipError_t lauum_block(int dtype, bool lower, i64 n, void* A, i64 lda, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (n > kTrtriMax || lda < n) return hipErrorInvalidValue;
    ELX_KERN_REAL_SWITCH(dtype, T, return launch_lauum(lower, n, static_cast<T*>(A), lda, s));
}

}  // namespace kern
}  // namespace elx
