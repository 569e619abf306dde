// El::LU / lu::SolveAfter / LinearSolve / Permutation through the drop-in header
// (include/El.hpp) on Device::CPU matrices over a 1x1 grid, against a
// hand-computed 3 x 3 case (every intermediate value is exact):
//   A = [1 1.5 5; 4 2 2; 2 3 2]:  step 0 swaps rows 0 and 1, step 1 rows 1 and 2,
//   P A = [4 2 2; 2 3 2; 1 1.5 5] = L U,  L = [1 . .; .5 1 .; .25 .5 1],
//   U = [4 2 2; . 2 1; . . 4],  A [1; 2; 3] = [19; 14; 14].
#include <El.hpp>

#include <cstdio>
#include <cstring>
#include <string>
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
    const std::vector<double> a = {1, 4, 2, 1.5, 2, 3, 5, 2, 2};         // column-major
    const std::vector<double> lu = {4, 0.5, 0.25, 2, 2, 0.5, 2, 1, 4};   // L below, U on and above
    const std::vector<double> b = {19, 14, 14};
    const std::vector<Int> swaps = {1, 2, 2}, expl = {1, 2, 0};

    {  // DistMatrix: the factors, the permutation, the solves
        DM<double> A(3, 3, g), B(3, 1, g);
        El::DistPermutation P;
        A.SetLocalBlock(a.data(), 3);
        El::LU(A, P);
        EXPECT(Local(A) == lu);
        EXPECT(P.Height() == 3 && P.SwapDests() == swaps && P.ExplicitVector() == expl && !P.Parity());

        B.SetLocalBlock(b.data(), 3);
        El::lu::SolveAfter(El::NORMAL, A, P, B);
        EXPECT(Local(B) == (std::vector<double>{1, 2, 3}));
        // A^T [1; 2; 3] = [15; 14.5; 15]
        const std::vector<double> bt = {15, 14.5, 15};
        B.SetLocalBlock(bt.data(), 3);
        El::lu::SolveAfter(El::TRANSPOSE, A, P, B);
        EXPECT(Local(B) == (std::vector<double>{1, 2, 3}));

        // P B = [b1; b2; b0] and back
        B.SetLocalBlock(b.data(), 3);
        P.PermuteRows(B);
        EXPECT(Local(B) == (std::vector<double>{14, 14, 19}));
        const std::vector<double> c = {7, 8, 9};
        B.SetLocalBlock(c.data(), 3);
        P.PermuteRows(B);
        EXPECT(Local(B) == (std::vector<double>{8, 9, 7}));
        P.InversePermuteRows(B);
        EXPECT(Local(B) == c);

        DM<double> R(3, 2, g);
        bool threw = false;
        try { El::lu::SolveAfter(El::NORMAL, R, P, B); }
        catch (const El::LogicError&) { threw = true; }
        EXPECT(threw);  // A must be square
    }
    {  // LinearSolve leaves A as it was
        DM<double> A(3, 3, g), B(3, 1, g);
        A.SetLocalBlock(a.data(), 3);
        B.SetLocalBlock(b.data(), 3);
        El::LinearSolve(A, B);
        EXPECT(Local(B) == (std::vector<double>{1, 2, 3}));
        EXPECT(Local(A) == a);
    }
    {  // Matrix
        El::Matrix<double, kDev> A(3, 3), B(3, 1);
        for (Int j = 0; j < 3; ++j)
            for (Int i = 0; i < 3; ++i) A.Set(i, j, a[i + 3 * j]);
        El::Permutation P;
        El::LU(A, P);
        for (Int j = 0; j < 3; ++j)
            for (Int i = 0; i < 3; ++i) EXPECT(A.Get(i, j) == lu[i + 3 * j]);
        EXPECT(P.SwapDests() == swaps);
        for (Int i = 0; i < 3; ++i) B.Set(i, 0, 7 + i);
        P.PermuteRows(B);
        EXPECT(B.Get(0, 0) == 8 && B.Get(1, 0) == 9 && B.Get(2, 0) == 7);
    }
    {  // singular: column 1 is exactly zero
        DM<double> A(3, 3, g);
        std::vector<double> bad = a;
        bad[3] = bad[4] = bad[5] = 0;
        A.SetLocalBlock(bad.data(), 3);
        El::DistPermutation P;
        std::string what;
        try { El::LU(A, P); }
        catch (const El::SingularMatrixException& e) { what = e.what(); }
        EXPECT(what.find("column 2") != std::string::npos);
        // and the library is still usable
        A.SetLocalBlock(a.data(), 3);
        El::LU(A, P);
        EXPECT(Local(A) == lu);
    }
    El::Finalize();
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("El::LU API test OK\n");
    return 0;
}
