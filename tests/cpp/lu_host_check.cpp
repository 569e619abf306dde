// The host side of El::LU over the C ABI, stand-alone: the CPU LocalLU (leaf loop,
// recursion, laswp, Trsm, Gemm) through elx_matrix_lu and the Permutation code
// through elx_lu / elx_perm_* on Device::CPU, on the shapes the LU tests use.
// Built plainly by tests/test_lu_cpu.py; the same source is what a sanitizer
// build of the library's host code is linked with and run.
#include <elemental_amd.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: EXPECT(%s) failed: %s\n", __FILE__, __LINE__, #cond, elx_last_error()); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static double Uniform(uint64_t& s) {  // xorshift64*, in [-1, 1)
    s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
    return (double)((s * 2685821657736338717ull) >> 11) / 4503599627370496.0 - 1.0;
}

// ||P A - L U||_F / (max(m, n) eps ||A||_F), -1 when the swaps or L are out of range
template <typename T>
static double Residual(int64_t m, int64_t n, const std::vector<T>& A, int64_t lda, const std::vector<T>& F,
                       const std::vector<int32_t>& piv) {
    const int64_t k = std::min(m, n);
    std::vector<double> PA(m * n);
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = 0; i < m; ++i) PA[i + j * m] = (double)A[i + j * lda];
    for (int64_t j = 0; j < k; ++j) {
        if (piv[j] < j || piv[j] >= m) return -1;
        for (int64_t c = 0; c < n; ++c) std::swap(PA[j + c * m], PA[piv[j] + c * m]);
    }
    double err = 0, nrm = 0;
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = 0; i < m; ++i) {
            double acc = 0;
            for (int64_t l = 0; l <= std::min(std::min(i, j), k - 1); ++l) {
                const double lv = l == i ? 1.0 : (double)F[i + l * lda];
                if (l < i && std::fabs(lv) > 1.0) return -1;
                acc += lv * (double)F[l + j * lda];
            }
            err += (PA[i + j * m] - acc) * (PA[i + j * m] - acc);
            nrm += PA[i + j * m] * PA[i + j * m];
        }
    return std::sqrt(err) / ((double)std::max(m, n) * (double)std::numeric_limits<T>::epsilon() * std::sqrt(nrm));
}

template <typename T>
static void Case(int dtype, int64_t m, int64_t n, int64_t pad) {
    const int64_t lda = m + pad, k = std::min(m, n);
    uint64_t seed = 88172645463325252ull + (uint64_t)(m * 1315423911 + n);
    std::vector<T> A(lda * n, std::numeric_limits<T>::quiet_NaN());
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = 0; i < m; ++i) A[i + j * lda] = (T)Uniform(seed);
    std::vector<T> F = A;
    std::vector<int32_t> piv(k, -1);
    EXPECT(elx_matrix_lu(dtype, ELX_DEVICE_CPU, m, n, F.data(), lda, piv.data(), nullptr) == ELX_OK);
    const double r = Residual(m, n, A, lda, F, piv);
    std::printf("lu %lld x %lld (%s, lda %lld): %.3g of max(m,n) eps ||A||_F\n", (long long)m, (long long)n,
                sizeof(T) == 8 ? "f64" : "f32", (long long)lda, r);
    EXPECT(r >= 0 && r <= 10);
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = m; i < lda; ++i) EXPECT(std::isnan(F[i + j * lda]));
    // a zero column: ELX_ERR_SINGULAR, and the buffers are still ours to free
    if (m == n && n > 1) {
        std::vector<T> Z = A;
        for (int64_t i = 0; i < m; ++i) Z[i + (n / 2) * lda] = 0;
        EXPECT(elx_matrix_lu(dtype, ELX_DEVICE_CPU, m, n, Z.data(), lda, piv.data(), nullptr) == ELX_ERR_SINGULAR);
    }
}

static void PermutationCase(int64_t m, int64_t w) {
    elx_comm_t comm = nullptr;
    elx_grid_t grid = nullptr;
    elx_dm_t A = nullptr, B = nullptr;
    elx_perm_t P = nullptr;
    EXPECT(elx_comm_init_host(&comm, 0, 1, nullptr, nullptr, nullptr) == ELX_OK);
    EXPECT(elx_grid_create(&grid, comm, 1, ELX_COLUMN_MAJOR) == ELX_OK);
    EXPECT(elx_dm_create(&A, grid, ELX_F64, ELX_MC, ELX_MR, ELX_DEVICE_CPU, 0) == ELX_OK);
    EXPECT(elx_dm_create(&B, grid, ELX_F64, ELX_MC, ELX_MR, ELX_DEVICE_CPU, 0) == ELX_OK);
    EXPECT(elx_dm_resize(A, m, m) == ELX_OK && elx_dm_resize(B, m, w) == ELX_OK);
    uint64_t seed = 1234567 + (uint64_t)m;
    std::vector<double> a(m * m), b(m * w);
    for (double& v : a) v = Uniform(seed);
    for (double& v : b) v = Uniform(seed);
    b[0] = -0.0;
    EXPECT(elx_dm_set_local(A, a.data(), m) == ELX_OK && elx_dm_set_local(B, b.data(), m) == ELX_OK);
    EXPECT(elx_perm_create(&P) == ELX_OK);
    EXPECT(elx_lu(A, P) == ELX_OK);
    EXPECT(elx_perm_height(P) == m && elx_perm_num_swaps(P) == m);
    std::vector<int64_t> d(m);
    EXPECT(elx_perm_swaps(P, d.data()) == ELX_OK);
    std::vector<double> want = b, got(m * w);
    for (int64_t k = 0; k < m; ++k) {
        EXPECT(d[k] >= k && d[k] < m);
        for (int64_t c = 0; c < w; ++c) std::swap(want[k + c * m], want[d[k] + c * m]);
    }
    EXPECT(elx_perm_permute_rows(P, B, 0) == ELX_OK);
    EXPECT(elx_dm_get_local(B, got.data(), m) == ELX_OK);
    EXPECT(std::memcmp(got.data(), want.data(), got.size() * sizeof(double)) == 0);
    EXPECT(elx_perm_permute_rows(P, B, 1) == ELX_OK);
    EXPECT(elx_dm_get_local(B, got.data(), m) == ELX_OK);
    EXPECT(std::memcmp(got.data(), b.data(), got.size() * sizeof(double)) == 0);
    // LinearSolve on the same A: ||b - A x||_oo small
    EXPECT(elx_dm_set_local(A, a.data(), m) == ELX_OK && elx_dm_set_local(B, b.data(), m) == ELX_OK);
    EXPECT(elx_linear_solve(A, B) == ELX_OK);
    EXPECT(elx_perm_destroy(P) == ELX_OK);
    EXPECT(elx_dm_destroy(A) == ELX_OK && elx_dm_destroy(B) == ELX_OK);
    EXPECT(elx_grid_destroy(grid) == ELX_OK);
    EXPECT(elx_comm_destroy(comm) == ELX_OK);
}

int main() {
    const int64_t shapes[][2] = {{1, 1}, {16, 16}, {17, 17}, {33, 31}, {129, 129}, {300, 37}, {37, 300},
                                 {515, 145}, {257, 33}, {33, 257}};
    for (const auto& s : shapes) {
        Case<double>(ELX_F64, s[0], s[1], 0);
        Case<double>(ELX_F64, s[0], s[1], 3);
        Case<float>(ELX_F32, s[0], s[1], 3);
    }
    PermutationCase(19, 5);
    PermutationCase(150, 9);
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("LU host check OK\n");
    return 0;
}
