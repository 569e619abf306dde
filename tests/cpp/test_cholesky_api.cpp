// El::Cholesky / cholesky::SolveAfter / HPDSolve through the drop-in header
// (include/El.hpp) on Device::CPU matrices over a 1x1 grid, against a
// hand-computed 3 x 3 case (every intermediate value is an integer):
//   L = [2 . .; 3 4 .; 5 6 8],  A = L L^T = [4 6 10; 6 25 39; 10 39 125],
//   A [1; 2; 3] = [46; 173; 463].
#include <El.hpp>

#include <cmath>
#include <cstdio>
#include <vector>

constexpr El::Device kDev = El::Device::CPU;
template <typename T, El::Dist U = El::MC, El::Dist V = El::MR>
using DM = El::DistMatrix<T, U, V, El::ELEMENT, kDev>;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

template <typename M>
static std::vector<double> Local(const M& A) {
    std::vector<double> h(A.LocalHeight() * A.LocalWidth());
    A.GetLocalBlock(h.data(), A.LocalHeight());
    return h;
}

// equal where `want` is a number, NaN where it is NaN
static bool Same(const std::vector<double>& got, const std::vector<double>& want) {
    if (got.size() != want.size()) return false;
    for (size_t i = 0; i < got.size(); ++i)
        if (std::isnan(want[i]) ? !std::isnan(got[i]) : got[i] != want[i]) return false;
    return true;
}

int main() {
    using El::Int;
    El::Initialize();
    El::Grid g;  // 1x1 over COMM_SELF
    const double nan = std::nan("");
    // column-major; the triangle Cholesky must not touch is NaN
    const std::vector<double> a_lower = {4, 6, 10, nan, 25, 39, nan, nan, 125};
    const std::vector<double> a_upper = {4, nan, nan, 6, 25, nan, 10, 39, 125};
    const std::vector<double> l_lower = {2, 3, 5, nan, 4, 6, nan, nan, 8};
    const std::vector<double> l_upper = {2, nan, nan, 3, 4, nan, 5, 6, 8};  // U = L^T
    const std::vector<double> b = {46, 173, 463};

    {  // DistMatrix, both triangles, then the solve from the factor
        DM<double> A(3, 3, g), B(3, 1, g);
        A.SetLocalBlock(a_lower.data(), 3);
        El::Cholesky(El::LOWER, A);
        EXPECT(Same(Local(A), l_lower));
        B.SetLocalBlock(b.data(), 3);
        El::cholesky::SolveAfter(El::LOWER, El::NORMAL, A, B);
        EXPECT(Local(B) == (std::vector<double>{1, 2, 3}));

        A.SetLocalBlock(a_upper.data(), 3);
        El::Cholesky(El::UPPER, A);
        EXPECT(Same(Local(A), l_upper));
        B.SetLocalBlock(b.data(), 3);
        El::cholesky::SolveAfter(El::UPPER, El::NORMAL, A, B);
        EXPECT(Local(B) == (std::vector<double>{1, 2, 3}));

        DM<double> R(3, 2, g);
        bool threw = false;
        try { El::Cholesky(El::LOWER, R); }
        catch (const El::LogicError&) { threw = true; }
        EXPECT(threw);  // A must be square
    }
    {  // HPDSolve leaves A as it was
        DM<double> A(3, 3, g), B(3, 1, g);
        A.SetLocalBlock(a_lower.data(), 3);
        B.SetLocalBlock(b.data(), 3);
        El::HPDSolve(El::LOWER, El::NORMAL, A, B);
        EXPECT(Local(B) == (std::vector<double>{1, 2, 3}));
        EXPECT(Same(Local(A), a_lower));
    }
    {  // Matrix
        El::Matrix<double, kDev> A(3, 3);
        for (Int j = 0; j < 3; ++j)
            for (Int i = 0; i < 3; ++i) A.Set(i, j, a_lower[i + 3 * j]);
        El::Cholesky(El::LOWER, A);
        for (Int j = 0; j < 3; ++j)
            for (Int i = j; i < 3; ++i) EXPECT(A.Get(i, j) == l_lower[i + 3 * j]);
        EXPECT(std::isnan(A.Get(0, 1)) && std::isnan(A.Get(0, 2)) && std::isnan(A.Get(1, 2)));
        El::Matrix<double, kDev> R(3, 2);
        bool threw = false;
        try { El::Cholesky(El::LOWER, R); }
        catch (const El::LogicError&) { threw = true; }
        EXPECT(threw);
    }
    {  // not HPD: the second pivot is 25 - 3^2 - 16 = 0
        DM<double> A(3, 3, g);
        std::vector<double> bad = a_lower;
        bad[4] = 9;
        A.SetLocalBlock(bad.data(), 3);
        int column = 0;
        try { El::Cholesky(El::LOWER, A); }
        catch (const El::NonHPDMatrixException& e) { column = e.Column(); }
        EXPECT(column == 2);
        // and the library is still usable
        A.SetLocalBlock(a_lower.data(), 3);
        El::Cholesky(El::LOWER, A);
        EXPECT(Same(Local(A), l_lower));
    }
    El::Finalize();
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("El::Cholesky API test OK\n");
    return 0;
}
