// The host side of the Level-2 routines over the C ABI, stand-alone: the CPU loops
// behind elx_matrix_gemv / ger / symv / symv_accumulate / syr / syr2 on heap buffers of
// exactly the size an operand needs (lda (n - 1) + m elements, 1 + (len - 1) inc for a
// vector), so a read or write past an operand lands outside its allocation, and the
// DistMatrix drivers (elx_gemv, elx_ger, elx_symv, elx_syr, elx_syr2) on Device::CPU.
// Built plainly by tests/test_level2_cpu.py; the same source is what a sanitizer build
// of the library's host code is linked with and run.
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

template <typename T> struct Code;
template <> struct Code<double> { static constexpr int v = ELX_F64; };
template <> struct Code<float> { static constexpr int v = ELX_F32; };

template <typename T>
static std::vector<T> Vector(int64_t len, int64_t inc, uint64_t& s) {
    std::vector<T> v(len > 0 ? 1 + (len - 1) * inc : 0, std::numeric_limits<T>::quiet_NaN());
    for (int64_t i = 0; i < len; ++i) v[i * inc] = (T)Uniform(s);
    return v;
}
template <typename T>
static std::vector<T> Matrix(int64_t m, int64_t n, int64_t lda, uint64_t& s) {
    std::vector<T> A(m > 0 && n > 0 ? lda * (n - 1) + m : 0, std::numeric_limits<T>::quiet_NaN());
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = 0; i < m; ++i) A[i + j * lda] = (T)Uniform(s);
    return A;
}

template <typename T>
static void CheckLocal(int64_t m, int64_t n, int64_t pad, int64_t inc) {
    const int dt = Code<T>::v, dev = ELX_DEVICE_CPU;
    const double eps = std::numeric_limits<T>::epsilon();
    uint64_t s = 88172645463325252ull + (uint64_t)(m * 131 + n);
    const int64_t lda = std::max<int64_t>(m, 1) + pad;
    const std::vector<T> A = Matrix<T>(m, n, lda, s);
    for (int trans = 0; trans < 2; ++trans) {
        const int64_t k = trans ? m : n, ylen = trans ? n : m;
        const std::vector<T> x = Vector<T>(k, inc, s);
        std::vector<T> y = Vector<T>(ylen, inc, s);
        const std::vector<T> y0 = y;
        EXPECT(elx_matrix_gemv(dt, dev, trans ? ELX_TRANSPOSE : ELX_NORMAL, m, n, 0.75, A.data(), lda, x.data(), inc, -0.5,
                               y.data(), inc, nullptr) == ELX_OK);
        for (int64_t i = 0; i < ylen; ++i) {
            double ref = -0.5 * (double)y0[i * inc], S = 0.5 * std::fabs((double)y0[i * inc]);
            for (int64_t l = 0; l < k; ++l) {
                const double a = trans ? (double)A[l + i * lda] : (double)A[i + l * lda];
                ref += 0.75 * a * (double)x[l * inc];
                S += 0.75 * std::fabs(a * (double)x[l * inc]);
            }
            EXPECT(std::fabs((double)y[i * inc] - ref) <= (double)(k + 3) * eps * S);
        }
    }
    {  // Ger
        std::vector<T> B = A;
        const std::vector<T> x = Vector<T>(m, inc, s), y = Vector<T>(n, inc, s);
        EXPECT(elx_matrix_ger(dt, dev, m, n, 0.75, x.data(), inc, y.data(), inc, B.data(), lda, nullptr) == ELX_OK);
        for (int64_t j = 0; j < n; ++j)
            for (int64_t i = 0; i < m; ++i) {
                const double u = 0.75 * (double)x[i * inc] * (double)y[j * inc];
                EXPECT(std::fabs((double)B[i + j * lda] - ((double)A[i + j * lda] + u)) <=
                       4 * eps * (std::fabs((double)A[i + j * lda]) + std::fabs(u)));
            }
    }
    if (m == 0 || n == 0) return;
    if (m != n) {
        // the trapezoid form with a rank's index map: rows 1, 3, 5, ..., columns 0, 3, 6, ...
        for (int uplo = ELX_LOWER; uplo <= ELX_UPPER; ++uplo) {
            const std::vector<T> xr = Vector<T>(m, 1, s), xc = Vector<T>(n, inc, s);
            std::vector<T> zr(xr.size(), (T)0), zc(xc.size(), (T)0);
            EXPECT(elx_matrix_symv_accumulate(dt, dev, uplo, m, n, 1.0, A.data(), lda, xr.data(), 1, xc.data(), inc,
                                              zr.data(), 1, zc.data(), inc, 1, 2, 0, 3, nullptr) == ELX_OK);
            std::vector<double> rr(m, 0.0), rc(n, 0.0);
            for (int64_t j = 0; j < n; ++j)
                for (int64_t i = 0; i < m; ++i) {
                    const int64_t gi = 1 + 2 * i, gj = 3 * j;
                    if (uplo == ELX_LOWER ? gi >= gj : gi <= gj) rr[i] += (double)A[i + j * lda] * (double)xc[j * inc];
                    if (uplo == ELX_LOWER ? gi > gj : gi < gj) rc[j] += (double)A[i + j * lda] * (double)xr[i];
                }
            for (int64_t i = 0; i < m; ++i) EXPECT(std::fabs((double)zr[i] - rr[i]) <= (double)(n + 3) * eps * (double)n);
            for (int64_t j = 0; j < n; ++j)
                EXPECT(std::fabs((double)zc[j * inc] - rc[j]) <= (double)(m + 3) * eps * (double)m);
        }
        return;
    }
    for (int uplo = ELX_LOWER; uplo <= ELX_UPPER; ++uplo) {
        const auto stored = [&](int64_t i, int64_t j) { return uplo == ELX_LOWER ? i >= j : i <= j; };
        const auto sym = [&](int64_t i, int64_t j) { return (double)(stored(i, j) ? A[i + j * lda] : A[j + i * lda]); };
        const std::vector<T> x = Vector<T>(n, inc, s), w = Vector<T>(n, inc, s);
        std::vector<T> y = Vector<T>(n, inc, s);
        const std::vector<T> y0 = y;
        EXPECT(elx_matrix_symv(dt, dev, uplo, n, 0.75, A.data(), lda, x.data(), inc, -0.5, y.data(), inc, nullptr) ==
               ELX_OK);
        for (int64_t i = 0; i < n; ++i) {
            double ref = -0.5 * (double)y0[i * inc], S = 0.5 * std::fabs((double)y0[i * inc]);
            for (int64_t j = 0; j < n; ++j) {
                ref += 0.75 * sym(i, j) * (double)x[j * inc];
                S += 0.75 * std::fabs(sym(i, j) * (double)x[j * inc]);
            }
            EXPECT(std::fabs((double)y[i * inc] - ref) <= (double)(n + 3) * eps * S);
        }
        std::vector<T> B = A, C = A;
        EXPECT(elx_matrix_syr(dt, dev, uplo, n, 0.75, x.data(), inc, B.data(), lda, nullptr) == ELX_OK);
        EXPECT(elx_matrix_syr2(dt, dev, uplo, n, 0.75, x.data(), inc, w.data(), inc, C.data(), lda, nullptr) == ELX_OK);
        for (int64_t j = 0; j < n; ++j)
            for (int64_t i = 0; i < n; ++i) {
                const double a = (double)A[i + j * lda], xi = (double)x[i * inc], xj = (double)x[j * inc];
                const double wi = (double)w[i * inc], wj = (double)w[j * inc];
                if (!stored(i, j)) {
                    EXPECT(B[i + j * lda] == A[i + j * lda] && C[i + j * lda] == A[i + j * lda]);
                    continue;
                }
                EXPECT(std::fabs((double)B[i + j * lda] - (a + 0.75 * xi * xj)) <=
                       4 * eps * (std::fabs(a) + std::fabs(xi * xj)));
                EXPECT(std::fabs((double)C[i + j * lda] - (a + 0.75 * (xi * wj + wi * xj))) <=
                       4 * eps * (std::fabs(a) + std::fabs(xi * wj) + std::fabs(wi * xj)));
            }
    }
}

// the drivers on a 1 x 1 grid of Device::CPU matrices, vectors as columns and as rows
static void CheckDrivers(int64_t m, int64_t n) {
    elx_comm_t comm = nullptr;
    elx_grid_t grid = nullptr;
    EXPECT(elx_comm_world(&comm) == ELX_OK);
    EXPECT(elx_grid_create(&grid, comm, 1, ELX_COLUMN_MAJOR) == ELX_OK);
    const auto make = [&](int64_t h, int64_t w, int U, int V, uint64_t seed) {
        elx_dm_t D = nullptr;
        EXPECT(elx_dm_create(&D, grid, ELX_F64, U, V, ELX_DEVICE_CPU, 0) == ELX_OK);
        EXPECT(elx_dm_resize(D, h, w) == ELX_OK);
        EXPECT(elx_dm_fill_hash(D, seed, 0.0, 1.0) == ELX_OK);
        return D;
    };
    const auto get = [&](elx_dm_t D, int64_t h, int64_t w) {
        std::vector<double> v(h * w);
        elx_dm_t S = nullptr;
        EXPECT(elx_dm_create(&S, grid, ELX_F64, ELX_STAR, ELX_STAR, ELX_DEVICE_CPU, 0) == ELX_OK);
        EXPECT(elx_dm_copy(S, D) == ELX_OK);
        if (!v.empty()) EXPECT(elx_dm_get_local(S, v.data(), h) == ELX_OK);
        elx_dm_destroy(S);
        return v;
    };
    const double eps = std::numeric_limits<double>::epsilon();
    for (int row = 0; row < 2; ++row) {
        elx_dm_t A = make(m, n, ELX_MC, ELX_MR, 1), S = make(m, m, ELX_MC, ELX_MR, 2);
        elx_dm_t x = row ? make(1, n, ELX_MC, ELX_MR, 3) : make(n, 1, ELX_VC, ELX_STAR, 3);
        elx_dm_t y = row ? make(1, m, ELX_MC, ELX_MR, 4) : make(m, 1, ELX_MC, ELX_MR, 4);
        elx_dm_t v = row ? make(1, m, ELX_MC, ELX_MR, 5) : make(m, 1, ELX_MC, ELX_MR, 5);
        const std::vector<double> a = get(A, m, n), s0 = get(S, m, m), xv = get(x, row ? 1 : n, row ? n : 1);
        const std::vector<double> y0 = get(y, row ? 1 : m, row ? m : 1), vv = get(v, row ? 1 : m, row ? m : 1);
        EXPECT(elx_gemv(ELX_NORMAL, 0.75, A, x, -0.5, y) == ELX_OK);
        const std::vector<double> y1 = get(y, row ? 1 : m, row ? m : 1);
        for (int64_t i = 0; i < m; ++i) {
            double ref = -0.5 * y0[i];
            for (int64_t j = 0; j < n; ++j) ref += 0.75 * a[i + j * m] * xv[j];
            EXPECT(std::fabs(y1[i] - ref) <= (double)(n + 3) * eps * (double)(n + 1));
        }
        EXPECT(elx_gemv(ELX_TRANSPOSE, 1.0, A, v, 0.0, x) == ELX_OK);
        const std::vector<double> x1 = get(x, row ? 1 : n, row ? n : 1);
        for (int64_t j = 0; j < n; ++j) {
            double ref = 0;
            for (int64_t i = 0; i < m; ++i) ref += a[i + j * m] * vv[i];
            EXPECT(std::fabs(x1[j] - ref) <= (double)(m + 3) * eps * (double)m);
        }
        EXPECT(elx_symv(ELX_LOWER, 1.0, S, v, 0.0, y, 0) == ELX_OK);
        const std::vector<double> y2 = get(y, row ? 1 : m, row ? m : 1);
        for (int64_t i = 0; i < m; ++i) {
            double ref = 0;
            for (int64_t j = 0; j < m; ++j) ref += (i >= j ? s0[i + j * m] : s0[j + i * m]) * vv[j];
            EXPECT(std::fabs(y2[i] - ref) <= (double)(m + 3) * eps * (double)m);
        }
        EXPECT(elx_ger(1.0, v, x, A) == ELX_OK);
        const std::vector<double> a1 = get(A, m, n);
        for (int64_t j = 0; j < n; ++j)
            for (int64_t i = 0; i < m; ++i) EXPECT(std::fabs(a1[i + j * m] - (a[i + j * m] + vv[i] * x1[j])) <= 8 * eps);
        EXPECT(elx_syr(ELX_UPPER, 1.0, v, S, 0) == ELX_OK);
        EXPECT(elx_syr2(ELX_LOWER, 1.0, v, y, S, 0) == ELX_OK);
        const std::vector<double> s1 = get(S, m, m);
        for (int64_t j = 0; j < m; ++j)
            for (int64_t i = 0; i < m; ++i) {
                double ref = s0[i + j * m];
                if (i <= j) ref += vv[i] * vv[j];
                if (i >= j) ref += vv[i] * y2[j] + y2[i] * vv[j];
                EXPECT(std::fabs(s1[i + j * m] - ref) <= 16 * eps * (double)m);
            }
        for (elx_dm_t D : {A, S, x, y, v}) elx_dm_destroy(D);
    }
    elx_grid_destroy(grid);
}

int main() {
    EXPECT(elx_initialize() == ELX_OK);
    const int64_t R = elx_level2_gemv_rows(), C = elx_level2_gemv_cols(), T = elx_level2_symv_tile();
    EXPECT(R > 0 && C > 0 && T > 0);
    const int64_t shapes[][2] = {{1, 1}, {2, 1}, {1, 2}, {63, 65}, {65, 63}, {T - 1, T - 1}, {T + 1, T + 1}, {R + 1, 3},
                                 {3, C + 1}, {2 * T + 1, 2 * T + 1}, {0, 5}, {5, 0}};
    for (const auto& sh : shapes)
        for (int64_t pad = 0; pad <= 3; pad += 3) {
            CheckLocal<double>(sh[0], sh[1], pad, pad ? 3 : 1);
            CheckLocal<float>(sh[0], sh[1], pad, pad ? 1 : 3);
        }
    CheckDrivers(37, 29);
    CheckDrivers(1, 1);
    EXPECT(elx_finalize() == ELX_OK);
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("Level-2 host check OK\n");
    return 0;
}
