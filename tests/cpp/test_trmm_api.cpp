// El::Trmm / El::LocalTrmm through the drop-in header (include/El.hpp) on
// Device::CPU matrices over a 1x1 grid, against a hand-computed 3 x 3 case:
//   L = [2 . .; 3 4 .; 5 6 7],  B = [1 2; 3 4; 5 6],  L B = [2 4; 15 22; 58 76].
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

int main() {
    using El::Int;
    El::Initialize();
    El::Grid g;  // 1x1 over COMM_SELF
    const double nan = std::nan("");
    // column-major; the triangle Trmm must not read is NaN
    const std::vector<double> lower = {2, 3, 5, nan, 4, 6, nan, nan, 7};
    const std::vector<double> upper = {2, nan, nan, 3, 4, nan, 5, 6, 7};  // = lower^T
    const std::vector<double> b = {1, 3, 5, 2, 4, 6};

    {  // DistMatrix: B := 2 L B
        DM<double> A(3, 3, g), B(3, 2, g);
        A.SetLocalBlock(lower.data(), 3);
        B.SetLocalBlock(b.data(), 3);
        El::Trmm(El::LEFT, El::LOWER, El::NORMAL, El::NON_UNIT, 2.0, A, B);
        EXPECT(Local(B) == (std::vector<double>{4, 30, 116, 8, 44, 152}));
        // the same product from the upper storage, transposed
        A.SetLocalBlock(upper.data(), 3);
        B.SetLocalBlock(b.data(), 3);
        El::Trmm(El::LEFT, El::UPPER, El::TRANSPOSE, El::NON_UNIT, 2.0, A, B);
        EXPECT(Local(B) == (std::vector<double>{4, 30, 116, 8, 44, 152}));
        DM<double> R(3, 2, g);
        bool threw = false;
        try { El::Trmm(El::LEFT, El::LOWER, El::NORMAL, El::NON_UNIT, 1.0, R, B); }
        catch (const El::LogicError&) { threw = true; }
        EXPECT(threw);  // Triangular matrix must be square
    }
    {  // Matrix, RIGHT: C (2 x 3) := C U^T = C L, C = [1 2 3; 4 5 6] -> [23 26 21; 53 56 42]
        El::Matrix<double, kDev> U(3, 3), C(2, 3);
        for (Int j = 0; j < 3; ++j)
            for (Int i = 0; i < 3; ++i) U.Set(i, j, upper[i + 3 * j]);
        for (Int j = 0; j < 3; ++j)
            for (Int i = 0; i < 2; ++i) C.Set(i, j, 1.0 + j + 3.0 * i);
        El::Trmm(El::RIGHT, El::UPPER, El::TRANSPOSE, El::NON_UNIT, 1.0, U, C);
        const double want[2][3] = {{23, 26, 21}, {53, 56, 42}};
        for (Int j = 0; j < 3; ++j)
            for (Int i = 0; i < 2; ++i) EXPECT(C.Get(i, j) == want[i][j]);
        bool threw = false;
        try { El::Trmm(El::LEFT, El::UPPER, El::NORMAL, El::NON_UNIT, 1.0, U, C); }
        catch (const El::LogicError&) { threw = true; }
        EXPECT(threw);  // Nonconformal Trmm
    }
    {  // LocalTrmm: A [*,*], B [*,VR]; UNIT: the diagonal counts as 1 -> [1 2; 6 10; 28 40]
        DM<double, El::STAR, El::STAR> A(3, 3, g);
        DM<double, El::STAR, El::VR> B(3, 2, g);
        std::vector<double> unit_lower = lower;
        unit_lower[0] = unit_lower[4] = unit_lower[8] = nan;
        A.SetLocalBlock(unit_lower.data(), 3);
        B.SetLocalBlock(b.data(), 3);
        El::LocalTrmm(El::LEFT, El::LOWER, El::NORMAL, El::UNIT, 1.0, A, B);
        EXPECT(Local(B) == (std::vector<double>{1, 6, 28, 2, 10, 40}));
        // B's dimension that meets the triangle must be STAR (Trmm.cpp:99-102)
        DM<double> Bad(3, 2, g);
        bool threw = false;
        try { El::LocalTrmm(El::LEFT, El::LOWER, El::NORMAL, El::UNIT, 1.0, A, Bad); }
        catch (const El::LogicError&) { threw = true; }
        EXPECT(threw);
        DM<double, El::VC, El::STAR> Br(2, 3, g);
        threw = false;
        try { El::LocalTrmm(El::RIGHT, El::LOWER, El::NORMAL, El::UNIT, 1.0, A, Br); }
        catch (const El::LogicError&) { threw = true; }
        EXPECT(!threw);
    }
    El::Finalize();
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("El::Trmm API test OK\n");
    return 0;
}
