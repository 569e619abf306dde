// The host side of El::HermitianTridiag over the C ABI, stand-alone: the CPU
// column loop through elx_matrix_hermitian_tridiag and the drivers through
// elx_hermitian_tridiag / _apply_q / _explicit_condensed on Device::CPU, on the
// sizes the tests use.  Built plainly by tests/test_tridiag_cpu.py; the same source
// is what a sanitizer build of the library's host code is linked with and run.
#include <elemental_amd.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
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

// ||S - Q T Q^T||_F / (n eps ||S||_F) with Q T Q^T formed by applying the reflectors
// to T from both sides in double; -1 when a scalar is out of range
template <typename T>
static double Residual(bool lower, int64_t n, const std::vector<T>& A, const std::vector<T>& F, int64_t lda,
                       const std::vector<T>& tau) {
    std::vector<double> W(n * n, 0.0);
    for (int64_t i = 0; i < n; ++i) {
        W[i + i * n] = (double)F[i + i * lda];
        if (i + 1 < n) {
            const double e = lower ? (double)F[i + 1 + i * lda] : (double)F[i + (i + 1) * lda];
            W[i + 1 + i * n] = W[i + (i + 1) * n] = e;
        }
    }
    std::vector<double> v(n), z(n);
    // Q T Q^T: the last factor of Q first
    for (int64_t s = 0; s + 1 < n; ++s) {
        const int64_t k = lower ? n - 2 - s : s + 1;  // the reflector's column
        const double t = (double)tau[lower ? k : k - 1];
        if (!(t >= 1 && t <= 2)) return -1;
        std::fill(v.begin(), v.end(), 0.0);
        if (lower) {
            v[k + 1] = 1;
            for (int64_t i = k + 2; i < n; ++i) v[i] = (double)F[i + k * lda];
        } else {
            v[k - 1] = 1;
            for (int64_t i = 0; i < k - 1; ++i) v[i] = (double)F[i + k * lda];
        }
        for (int side = 0; side < 2; ++side) {  // W := H W, then W := W H
            for (int64_t c = 0; c < n; ++c) {
                double d = 0;
                for (int64_t i = 0; i < n; ++i) d += v[i] * (side == 0 ? W[i + c * n] : W[c + i * n]);
                z[c] = t * d;
            }
            for (int64_t c = 0; c < n; ++c)
                for (int64_t i = 0; i < n; ++i) (side == 0 ? W[i + c * n] : W[c + i * n]) -= v[i] * z[c];
        }
    }
    double err = 0, nrm = 0, amax = 0;
    auto sym = [&](int64_t i, int64_t j) {
        const bool stored = lower ? i >= j : i <= j;
        return (double)(stored ? A[i + j * lda] : A[j + i * lda]);
    };
    for (int64_t c = 0; c < n; ++c)
        for (int64_t i = 0; i < n; ++i) amax = std::max(amax, std::fabs(sym(i, c)));
    if (amax == 0) amax = 1;
    for (int64_t c = 0; c < n; ++c)
        for (int64_t i = 0; i < n; ++i) {
            const double a = sym(i, c) / amax, q = W[i + c * n] / amax;
            err += (a - q) * (a - q);
            nrm += a * a;
        }
    if (nrm == 0) return 0;
    return std::sqrt(err) / ((double)n * (double)std::numeric_limits<T>::epsilon() * std::sqrt(nrm));
}

template <typename T>
static void Case(int dtype, int uplo, int64_t n, int64_t pad, double scale = 1.0) {
    const bool lower = uplo == ELX_LOWER;
    const int64_t lda = std::max<int64_t>(1, n + pad), k = std::max<int64_t>(n - 1, 0);
    uint64_t seed = 88172645463325252ull + (uint64_t)(n * 1315423911);
    const T nan = std::numeric_limits<T>::quiet_NaN();
    std::vector<T> A(lda * std::max<int64_t>(n, 1), nan);
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = 0; i < n; ++i)
            if (lower ? i >= j : i <= j) A[i + j * lda] = (T)(Uniform(seed) * scale);  // the other triangle stays NaN
    std::vector<T> F = A, tau(k + 2, (T)-7);
    EXPECT(elx_matrix_hermitian_tridiag(dtype, ELX_DEVICE_CPU, uplo, n, F.data(), lda, tau.data() + 1, nullptr) ==
           ELX_OK);
    EXPECT(tau[0] == -7 && tau[k + 1] == -7);
    const std::vector<T> t(tau.begin() + 1, tau.end() - 1);
    const double r = Residual(lower, n, A, F, lda, t);
    std::printf("tridiag %c n = %lld (%s, lda %lld, scale %g): %.3g of n eps ||S||_F\n", lower ? 'L' : 'U',
                (long long)n, sizeof(T) == 8 ? "f64" : "f32", (long long)lda, scale, r);
    EXPECT(r >= 0 && r <= 10);
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = 0; i < lda; ++i)
            if (i >= n || (lower ? i < j : i > j)) EXPECT(std::isnan(F[i + j * lda]));
}

// elx_hermitian_tridiag, Q then Q^T on B, ExplicitCondensed on a 1 x 1 grid
static void DriverCase(int uplo, int64_t n, int64_t w) {
    elx_comm_t comm = nullptr;
    elx_grid_t grid = nullptr;
    elx_dm_t A = nullptr, B = nullptr, t = nullptr;
    EXPECT(elx_comm_init_host(&comm, 0, 1, nullptr, nullptr, nullptr) == ELX_OK);
    EXPECT(elx_grid_create(&grid, comm, 1, ELX_COLUMN_MAJOR) == ELX_OK);
    for (elx_dm_t* M : {&A, &B, &t})
        EXPECT(elx_dm_create(M, grid, ELX_F64, ELX_MC, ELX_MR, ELX_DEVICE_CPU, 0) == ELX_OK);
    EXPECT(elx_dm_resize(A, n, n) == ELX_OK && elx_dm_resize(B, n, w) == ELX_OK);
    uint64_t seed = 1234567 + (uint64_t)n;
    std::vector<double> a(n * n), b(n * w), got(n * w);
    for (double& v : a) v = Uniform(seed);
    for (double& v : b) v = Uniform(seed);
    EXPECT(elx_dm_set_local(A, a.data(), n) == ELX_OK && elx_dm_set_local(B, b.data(), n) == ELX_OK);
    EXPECT(elx_set_blocksize(8) == ELX_OK);
    EXPECT(elx_hermitian_tridiag(uplo, A, t) == ELX_OK);
    EXPECT(elx_hermitian_tridiag_apply_q(ELX_LEFT, uplo, ELX_NORMAL, A, t, B) == ELX_OK);
    EXPECT(elx_hermitian_tridiag_apply_q(ELX_LEFT, uplo, ELX_ADJOINT, A, t, B) == ELX_OK);
    EXPECT(elx_dm_get_local(B, got.data(), n) == ELX_OK);
    double err = 0;
    for (size_t i = 0; i < got.size(); ++i) err = std::max(err, std::fabs(got[i] - b[i]));
    EXPECT(err <= 1e-12);
    EXPECT(elx_hermitian_tridiag_apply_q(ELX_RIGHT, uplo, ELX_NORMAL, A, t, B) == ELX_ERR_LOGIC);
    EXPECT(elx_dm_set_local(A, a.data(), n) == ELX_OK);
    EXPECT(elx_hermitian_tridiag_explicit_condensed(uplo, A) == ELX_OK);
    for (elx_dm_t M : {A, B, t}) EXPECT(elx_dm_destroy(M) == ELX_OK);
    EXPECT(elx_grid_destroy(grid) == ELX_OK);
    EXPECT(elx_comm_destroy(comm) == ELX_OK);
}

int main() {
    for (int uplo : {ELX_LOWER, ELX_UPPER}) {
        for (int64_t n : {0, 1, 2, 3, 16, 17, 33, 129, 300}) {
            Case<double>(ELX_F64, uplo, n, 0);
            Case<double>(ELX_F64, uplo, n, 3);
            Case<float>(ELX_F32, uplo, n, 3);
        }
        Case<double>(ELX_F64, uplo, 70, 0, std::ldexp(1.0, 500));
        Case<double>(ELX_F64, uplo, 70, 0, std::ldexp(1.0, -500));
        Case<float>(ELX_F32, uplo, 70, 0, std::ldexp(1.0, 50));
        Case<float>(ELX_F32, uplo, 70, 0, std::ldexp(1.0, -50));
        DriverCase(uplo, 19, 5);
        DriverCase(uplo, 45, 3);
    }
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("HermitianTridiag host check OK\n");
    return 0;
}
