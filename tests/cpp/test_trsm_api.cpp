// El::Trsm on Matrix through the drop-in header (include/El.hpp), Device::CPU,
// against a hand-computed 3 x 3 case:
//   L = [2 . .; 3 4 .; 5 6 7],  X = [1 2; 3 4; 5 6],  L X = [2 4; 15 22; 58 76].
#include <El.hpp>

#include <cmath>
#include <cstdio>
#include <vector>

constexpr El::Device kDev = El::Device::CPU;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

int main() {
    using El::Int;
    El::Initialize();
    const double nan = std::nan("");
    // column-major; the triangle Trsm must not read is NaN
    const std::vector<double> lower = {2, 3, 5, nan, 4, 6, nan, nan, 7};
    const std::vector<double> upper = {2, nan, nan, 3, 4, nan, 5, 6, 7};  // = lower^T
    auto fill = [](El::Matrix<double, kDev>& M, const std::vector<double>& v) {
        for (Int j = 0; j < M.Width(); ++j)
            for (Int i = 0; i < M.Height(); ++i) M.Set(i, j, v[i + M.Height() * j]);
    };
    {  // LEFT: L X = 2 B with B = L X / 2
        El::Matrix<double, kDev> A(3, 3), B(3, 2);
        fill(A, lower);
        fill(B, {1, 7.5, 29, 2, 11, 38});
        El::Trsm(El::LEFT, El::LOWER, El::NORMAL, El::NON_UNIT, 2.0, A, B);
        const double want[6] = {1, 3, 5, 2, 4, 6};
        for (Int j = 0; j < 2; ++j)
            for (Int i = 0; i < 3; ++i) EXPECT(B.Get(i, j) == want[i + 3 * j]);
        // the same system from the upper storage, transposed
        fill(A, upper);
        fill(B, {1, 7.5, 29, 2, 11, 38});
        El::Trsm(El::LEFT, El::UPPER, El::TRANSPOSE, El::NON_UNIT, 2.0, A, B);
        for (Int j = 0; j < 2; ++j)
            for (Int i = 0; i < 3; ++i) EXPECT(B.Get(i, j) == want[i + 3 * j]);
        // UNIT: the diagonal is not read and counts as 1: [1 . .; 3 1 .; 5 6 1] X = [1 2; 6 10; 28 40]
        std::vector<double> unit_lower = lower;
        unit_lower[0] = unit_lower[4] = unit_lower[8] = nan;
        fill(A, unit_lower);
        fill(B, {1, 6, 28, 2, 10, 40});
        El::Trsm(El::LEFT, El::LOWER, El::NORMAL, El::UNIT, 1.0, A, B);
        for (Int j = 0; j < 2; ++j)
            for (Int i = 0; i < 3; ++i) EXPECT(B.Get(i, j) == want[i + 3 * j]);
    }
    {  // RIGHT: X U^T = X L = C, X = [1 2 3; 4 5 6], C = [23 26 21; 53 56 42]
        El::Matrix<double, kDev> U(3, 3), C(2, 3);
        fill(U, upper);
        fill(C, {23, 53, 26, 56, 21, 42});
        El::Trsm(El::RIGHT, El::UPPER, El::TRANSPOSE, El::NON_UNIT, 1.0, U, C);
        for (Int j = 0; j < 3; ++j)
            for (Int i = 0; i < 2; ++i) EXPECT(C.Get(i, j) == 1.0 + j + 3.0 * i);
        bool threw = false;
        try { El::Trsm(El::LEFT, El::UPPER, El::NORMAL, El::NON_UNIT, 1.0, U, C); }
        catch (const El::LogicError&) { threw = true; }
        EXPECT(threw);  // Nonconformal Trsm
        El::Matrix<double, kDev> R(3, 2);
        threw = false;
        try { El::Trsm(El::RIGHT, El::UPPER, El::NORMAL, El::NON_UNIT, 1.0, R, C); }
        catch (const El::LogicError&) { threw = true; }
        EXPECT(threw);  // Triangular matrix must be square
    }
    {  // checkIfSingular (Trsm.cpp:62-68): an exact zero on a NON_UNIT diagonal
        El::Matrix<double, kDev> Z(3, 3), Y(3, 2);
        fill(Z, {2, 3, 5, nan, 0, 6, nan, nan, 7});
        fill(Y, {1, 2, 3, 4, 5, 6});
        bool threw = false;
        try { El::Trsm(El::LEFT, El::LOWER, El::NORMAL, El::NON_UNIT, 1.0, Z, Y, true); }
        catch (const El::SingularMatrixException&) { threw = true; }
        EXPECT(threw);
        EXPECT(Y.Get(1, 0) == 2.0);  // untouched
        El::Trsm(El::LEFT, El::LOWER, El::NORMAL, El::UNIT, 1.0, Z, Y, true);  // UNIT never reads it
        EXPECT(Y.Get(0, 0) == 1.0 && Y.Get(1, 0) == -1.0);
    }
    El::Finalize();
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("El::Trsm API test OK\n");
    return 0;
}
