// Cholesky factorization of one diagonal block: the leaf of the distributed
// Cholesky (LowerVariant3Unblocked on A11[*,*], LowerVariant3.hpp:17-50; the
// reference's GPU build calls the vendor solver through LocalGPUCholesky).
//
// One workgroup of NW waves factors the n x n block (n <= kPotrfMax) in LDS.
// The uplo triangle is staged once as the LOWER triangle of S (UPPER: the
// transpose is taken at this load and at the final store, A = U^T U is the same
// factorization of the same S), padded to np = a multiple of 16 with an
// identity, so every panel below is a full 16 columns and no loop has an edge.
// Per 16-column panel at p0:
//   panel   every lane owns one row of the panel in registers (16 values).
//           Lanes 0..15 of EVERY wave hold the 16 x 16 diagonal block (factored
//           redundantly per wave, so no wave waits for another), lanes 16..63
//           of wave w hold rows p0 + 16 + 48 w + (lane - 16).  Column j of the
//           diagonal block reaches the other lanes as wave-uniform values
//           (v_readlane): no LDS traffic and no barrier inside the panel.
//   update  S22 -= L21 L21^T on the 16 x 16 tiles on or below the diagonal,
//           four 16x16x4 MFMAs per tile, tiles dealt round-robin to the waves.
// Two workgroup barriers per panel instead of one per column.
//
// A pivot that is not > 0 (NaN included) stops the factorization: col0 + j + 1
// goes to *info (one ordinary store from one lane) and nothing is written back.
// A launch that finds *info != 0 returns at once.
#include "kernels.hpp"
#include "dtype_switch.hpp"
#include "mfma_tile.hpp"
#include "../common.hpp"

namespace elx {
namespace kern {
namespace {

constexpr int PW = 16;           // panel width = MFMA tile
constexpr int NW = 8;            // waves per workgroup
constexpr int NTHR = 64 * NW;
constexpr int ROWS_PER_WAVE = 64 - PW;  // rows below the diagonal block a wave owns per panel

__host__ __device__ constexpr i64 potrf_np(i64 n) { return (n + PW - 1) / PW * PW; }
__host__ __device__ constexpr i64 potrf_ld(i64 np) { return np + 1; }
template <typename T>
constexpr size_t potrf_lds(i64 n) {
    return (size_t)potrf_np(n) * potrf_ld(potrf_np(n)) * sizeof(T) + 16;  // + the failure word
}

__device__ __forceinline__ double read_lane(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float read_lane(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

template <typename T>
__global__ __launch_bounds__(NTHR) void potrf_kernel(bool lower, int n, T* A, i64 lda, int* info, int col0) {
    using M = Mfma<T>;
    using acc_t = typename M::acc_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (*info != 0) return;  // an earlier leaf failed (uniform: the whole workgroup leaves)

    const int np = (int)potrf_np(n), ld = (int)potrf_ld(np);
    T* S = reinterpret_cast<T*>(smem);
    int* fail = reinterpret_cast<int*>(smem + (size_t)np * ld * sizeof(T));
    auto at = [&](int i, int j) -> T& { return S[i + j * ld]; };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- stage: S(i,j) = A's triangle for n > i >= j, identity in the padding, 0 above
    if (tid == 0) *fail = 0;
    for (int c = wave; c < np; c += NW) {
        for (int r = lane; r < np; r += 64) {
            // LOWER: c is the column, r the row (unit stride in A and in S);
            // UPPER: A(c', r') with c' = r the row: S(c, r) = A[r + c*lda], r <= c
            const int i = lower ? r : c, j = lower ? c : r;
            T v = i == j ? T(1) : T(0);
            if (i >= j && i < n) v = A[(i64)r + (i64)c * lda];
            at(i, j) = v;
        }
    }
    __syncthreads();

    const int g = lane >> 4, c16 = lane & 15;
    for (int p0 = 0; p0 < np; p0 += PW) {
        // ---- panel
        const int below = np - p0 - PW;  // rows under the diagonal block
        const int row = lane < PW ? p0 + lane : p0 + PW + wave * ROWS_PER_WAVE + (lane - PW);
        const bool live = row < np;
        T a[PW];
        if (wave == 0 || wave * ROWS_PER_WAVE < below) {
#pragma unroll
            for (int k = 0; k < PW; ++k) a[k] = live ? at(row, p0 + k) : T(0);
            int bad = 0;
#pragma unroll
            for (int j = 0; j < PW; ++j) {
                if (bad) continue;  // wave-uniform (no break: the loop has to unroll, a[] stays in registers)
                const T d = read_lane(a[j], j);  // the pivot, held by the lane of diagonal row j
                if (!(d > T(0))) {
                    bad = j + 1;
                    continue;
                }
                const T sd = sqrt(d), inv = T(1) / sd;
                a[j] = lane == j ? sd : a[j] * inv;
#pragma unroll
                for (int k = j + 1; k < PW; ++k) a[k] -= a[j] * read_lane(a[j], k);
            }
            if (bad) {  // wave-uniform; every panel wave sees the same pivot
                if (tid == 0) {
                    *fail = 1;
                    if (*info == 0) *info = col0 + p0 + bad;
                }
            } else if (live && lane >= PW) {  // rows below: read and written by this wave alone
#pragma unroll
                for (int k = 0; k < PW; ++k) at(row, p0 + k) = a[k];
            }
        }
        __syncthreads();
        if (*fail) return;
        // the diagonal block goes back only now: the other panel waves read it
        // before the barrier, and the update below does not touch it
        if (wave == 0 && lane < PW) {
#pragma unroll
            for (int k = 0; k < PW; ++k)
                if (k <= lane) at(row, p0 + k) = a[k];
        }

        // ---- update: S(ti, tk) -= L(ti, panel) L(tk, panel)^T for tiles ti >= tk below the panel
        const int t0 = p0 / PW + 1, nt = np / PW;
        int cnt = 0;
        for (int ti = t0; ti < nt; ++ti) {
            for (int tk = t0; tk <= ti; ++tk, ++cnt) {
                if (cnt % NW != wave) continue;
                acc_t acc;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = at(ti * PW + M::row(g, r), tk * PW + c16);
#pragma unroll
                for (int s = 0; s < PW / 4; ++s) {
                    const T x = -at(ti * PW + c16, p0 + 4 * s + g);
                    const T y = at(tk * PW + c16, p0 + 4 * s + g);
                    acc = M::op(x, y, acc);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) at(ti * PW + M::row(g, r), tk * PW + c16) = acc[r];
            }
        }
        __syncthreads();
    }

    // ---- write back the triangle (UPPER: transposed, unit stride in A again)
    for (int c = wave; c < n; c += NW) {
        for (int r = lane; r < n; r += 64) {
            const int i = lower ? r : c, j = lower ? c : r;
            if (i >= j) A[(i64)r + (i64)c * lda] = at(i, j);
        }
    }
}

template <typename T>
hipError_t launch_potrf(bool lower, i64 n, T* A, i64 lda, int* info, int col0, hipStream_t s) {
    const size_t lds = potrf_lds<T>(n);
    if (lds > 64 * 1024) {  // beyond the default dynamic-LDS limit (gfx950: 160 KiB per workgroup)
        static const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&potrf_kernel<T>),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize,
                                                        (int)potrf_lds<T>(kPotrfMax));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((potrf_kernel<T>), dim3(1), dim3(NTHR), lds, s, lower, (int)n, A, lda, info, col0);
    return hipGetLastError();
}

static_assert(potrf_lds<double>(kPotrfMax) <= 160 * 1024, "kPotrfMax: the f64 block must fit one workgroup's LDS");

}  // namespace

hipError_t potrf_block(int dtype, bool lower, i64 n, void* A, i64 lda, int* info, int col0, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (n > kPotrfMax || lda < n || !info) return hipErrorInvalidValue;
    ELX_KERN_REAL_SWITCH(dtype, T,
                    return launch_potrf(lower, n, static_cast<T*>(A), lda, info, col0, s));
}

}  // namespace kern
}  // namespace elx
