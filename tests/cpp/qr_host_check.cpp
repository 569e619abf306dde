// The host side of El::QR over the C ABI, stand-alone: the CPU LocalQR (leaf loop,
// recursion, explicit reflectors, UT triangle, Trsm, Gemm, row scaling) through
// elx_matrix_qr and the distributed drivers through elx_qr / elx_qr_* on
// Device::CPU, on the shapes the QR tests use.  Built plainly by
// tests/test_qr_cpu.py; the same source is what a sanitizer build of the
// library's host code is linked with and run.
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

// ||A - Q R||_F / (max(m, n) eps ||A||_F) with Q R formed by applying H_0 .. H_{k-1}
// diag(d) to R in double; -1 when t, d or diag(R) are out of range
template <typename T>
static double Residual(int64_t m, int64_t n, const std::vector<T>& A, int64_t lda, const std::vector<T>& F,
                       const std::vector<T>& tau, const std::vector<T>& sig) {
    const int64_t k = std::min(m, n);
    std::vector<double> W(m * n, 0.0);  // diag(d) R, then the reflectors from the last to the first
    for (int64_t j = 0; j < k; ++j) {
        if (!(tau[j] >= 1 && tau[j] <= 2) || std::fabs((double)sig[j]) != 1 || !(F[j + j * lda] >= 0)) return -1;
    }
    for (int64_t c = 0; c < n; ++c)
        for (int64_t i = 0; i <= std::min(c, k - 1); ++i) W[i + c * m] = (double)sig[i] * (double)F[i + c * lda];
    for (int64_t j = k - 1; j >= 0; --j)
        for (int64_t c = 0; c < n; ++c) {
            double z = W[j + c * m];
            for (int64_t i = j + 1; i < m; ++i) z += (double)F[i + j * lda] * W[i + c * m];
            z *= (double)tau[j];
            W[j + c * m] -= z;
            for (int64_t i = j + 1; i < m; ++i) W[i + c * m] -= (double)F[i + j * lda] * z;
        }
    double err = 0, nrm = 0, amax = 0;  // sums of squares relative to the largest entry: no overflow
    for (int64_t c = 0; c < n; ++c)
        for (int64_t i = 0; i < m; ++i) amax = std::max(amax, std::fabs((double)A[i + c * lda]));
    if (amax == 0) amax = 1;
    for (int64_t c = 0; c < n; ++c)
        for (int64_t i = 0; i < m; ++i) {
            const double a = (double)A[i + c * lda] / amax, q = W[i + c * m] / amax;
            err += (a - q) * (a - q);
            nrm += a * a;
        }
    return std::sqrt(err) / ((double)std::max(m, n) * (double)std::numeric_limits<T>::epsilon() * std::sqrt(nrm));
}

template <typename T>
static void Case(int dtype, int64_t m, int64_t n, int64_t pad, double scale = 1.0) {
    const int64_t lda = m + pad, k = std::min(m, n);
    uint64_t seed = 88172645463325252ull + (uint64_t)(m * 1315423911 + n);
    std::vector<T> A(lda * n, std::numeric_limits<T>::quiet_NaN());
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = 0; i < m; ++i) A[i + j * lda] = (T)(Uniform(seed) * scale);
    std::vector<T> F = A, tau(k + 2, (T)-7), sig(k + 2, (T)-7);
    EXPECT(elx_matrix_qr(dtype, ELX_DEVICE_CPU, m, n, F.data(), lda, tau.data() + 1, sig.data() + 1, nullptr) == ELX_OK);
    EXPECT(tau[0] == -7 && tau[k + 1] == -7 && sig[0] == -7 && sig[k + 1] == -7);
    const std::vector<T> t(tau.begin() + 1, tau.end() - 1), d(sig.begin() + 1, sig.end() - 1);
    const double r = Residual(m, n, A, lda, F, t, d);
    std::printf("qr %lld x %lld (%s, lda %lld, scale %g): %.3g of max(m,n) eps ||A||_F\n", (long long)m, (long long)n,
                sizeof(T) == 8 ? "f64" : "f32", (long long)lda, scale, r);
    EXPECT(r >= 0 && r <= 10);
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = m; i < lda; ++i) EXPECT(std::isnan(F[i + j * lda]));
}

// elx_qr, apply Q then Q^T, the two solves, Explicit and LeastSquares on a 1 x 1 grid
static void DriverCase(int64_t m, int64_t n, int64_t w) {
    elx_comm_t comm = nullptr;
    elx_grid_t grid = nullptr;
    elx_dm_t A = nullptr, B = nullptr, X = nullptr, t = nullptr, d = nullptr, R = nullptr;
    EXPECT(elx_comm_init_host(&comm, 0, 1, nullptr, nullptr, nullptr) == ELX_OK);
    EXPECT(elx_grid_create(&grid, comm, 1, ELX_COLUMN_MAJOR) == ELX_OK);
    for (elx_dm_t* M : {&A, &B, &X, &t, &d, &R})
        EXPECT(elx_dm_create(M, grid, ELX_F64, ELX_MC, ELX_MR, ELX_DEVICE_CPU, 0) == ELX_OK);
    EXPECT(elx_dm_resize(A, m, n) == ELX_OK && elx_dm_resize(B, m, w) == ELX_OK);
    uint64_t seed = 1234567 + (uint64_t)m;
    std::vector<double> a(m * n), b(m * w), got(m * w), x(n * w);
    for (double& v : a) v = Uniform(seed);
    for (double& v : b) v = Uniform(seed);
    EXPECT(elx_dm_set_local(A, a.data(), m) == ELX_OK && elx_dm_set_local(B, b.data(), m) == ELX_OK);
    EXPECT(elx_set_blocksize(8) == ELX_OK);
    EXPECT(elx_qr(A, t, d) == ELX_OK);
    EXPECT(elx_qr_apply_q(ELX_LEFT, ELX_NORMAL, A, t, d, B) == ELX_OK);
    EXPECT(elx_qr_apply_q(ELX_LEFT, ELX_ADJOINT, A, t, d, B) == ELX_OK);
    EXPECT(elx_dm_get_local(B, got.data(), m) == ELX_OK);
    double err = 0;
    for (size_t i = 0; i < got.size(); ++i) err = std::max(err, std::fabs(got[i] - b[i]));
    EXPECT(err <= 1e-12);
    EXPECT(elx_qr_apply_q(ELX_RIGHT, ELX_NORMAL, A, t, d, B) == ELX_ERR_LOGIC);
    if (m >= n) {
        EXPECT(elx_qr_solve_after(ELX_NORMAL, A, t, d, B, X) == ELX_OK);
        EXPECT(elx_dm_get_local(X, x.data(), n) == ELX_OK);
        // the normal equations: A^T (A x - b) = 0
        double worst = 0;
        for (int64_t c = 0; c < w; ++c) {
            std::vector<double> r(m);
            for (int64_t i = 0; i < m; ++i) {
                r[i] = -b[i + c * m];
                for (int64_t l = 0; l < n; ++l) r[i] += a[i + l * m] * x[l + c * n];
            }
            for (int64_t l = 0; l < n; ++l) {
                double s = 0;
                for (int64_t i = 0; i < m; ++i) s += a[i + l * m] * r[i];
                worst = std::max(worst, std::fabs(s));
            }
        }
        EXPECT(worst <= 1e-11);
        EXPECT(elx_qr_solve_after(ELX_ADJOINT, A, t, d, X, B) == ELX_OK);
        EXPECT(elx_dm_set_local(A, a.data(), m) == ELX_OK);
        EXPECT(elx_least_squares(ELX_NORMAL, A, B, X) == ELX_OK);
    } else {
        EXPECT(elx_qr_solve_after(ELX_NORMAL, A, t, d, B, X) == ELX_ERR_LOGIC);
        EXPECT(elx_least_squares(ELX_NORMAL, A, B, X) == ELX_ERR_UNSUPPORTED);
    }
    EXPECT(elx_dm_resize(A, m, n) == ELX_OK && elx_dm_set_local(A, a.data(), m) == ELX_OK);
    EXPECT(elx_qr_explicit(A, R) == ELX_OK);
    EXPECT(elx_dm_resize(A, m, n) == ELX_OK && elx_dm_set_local(A, a.data(), m) == ELX_OK);
    EXPECT(elx_qr_explicit_triang(A) == ELX_OK);
    for (elx_dm_t M : {A, B, X, t, d, R}) EXPECT(elx_dm_destroy(M) == ELX_OK);
    EXPECT(elx_grid_destroy(grid) == ELX_OK);
    EXPECT(elx_comm_destroy(comm) == ELX_OK);
}

int main() {
    const int64_t shapes[][2] = {{1, 1}, {5, 3}, {16, 16}, {17, 17}, {33, 31}, {129, 129}, {300, 37}, {37, 300},
                                 {515, 145}, {257, 33}, {33, 257}};
    for (const auto& s : shapes) {
        Case<double>(ELX_F64, s[0], s[1], 0);
        Case<double>(ELX_F64, s[0], s[1], 3);
        Case<float>(ELX_F32, s[0], s[1], 3);
    }
    Case<double>(ELX_F64, 300, 37, 0, std::ldexp(1.0, 600));
    Case<double>(ELX_F64, 300, 37, 0, std::ldexp(1.0, -600));
    Case<float>(ELX_F32, 300, 37, 0, std::ldexp(1.0, 80));
    Case<float>(ELX_F32, 300, 37, 0, std::ldexp(1.0, -80));
    DriverCase(19, 19, 5);
    DriverCase(37, 20, 9);
    DriverCase(20, 37, 3);
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("QR host check OK\n");
    return 0;
}
