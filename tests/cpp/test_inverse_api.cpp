// El::TriangularInverse / Trtrmm / HPDInverse / LocalTriangularInverse through the
// drop-in header (include/El.hpp) on Device::CPU matrices over a 1x1 grid, against
// a hand-computed 3 x 3 case in which every value is a dyadic rational, so every
// operation order gives the same bits:
//   L = [2 . .; 4 1 .; 2 -2 4],   X = L^-1 = [1/2 . .; -2 1 .; -5/4 1/2 1/4],
//   L^T L = [24 0 8; 0 5 -8; 8 -8 16],   A = L L^T = [4 8 4; 8 17 6; 4 6 24],
//   A^-1 = X^T X = [93/16 -21/8 -5/16; -21/8 5/4 1/8; -5/16 1/8 1/16].
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

// the 3 x 3 column-major lower triangle as the upper triangle of its transpose
static std::vector<double> Transposed(const std::vector<double>& a) {
    std::vector<double> t(9);
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) t[j + 3 * i] = a[i + 3 * j];
    return t;
}

int main() {
    using El::Int;
    El::Initialize();
    El::Grid g;  // 1x1 over COMM_SELF
    const double nan = std::nan("");
    // column-major; the triangle that must not be touched is NaN
    const std::vector<double> l = {2, 4, 2, nan, 1, -2, nan, nan, 4};
    const std::vector<double> x = {0.5, -2, -1.25, nan, 1, 0.5, nan, nan, 0.25};
    const std::vector<double> ltl = {24, 0, 8, nan, 5, -8, nan, nan, 16};
    const std::vector<double> a = {4, 8, 4, nan, 17, 6, nan, nan, 24};
    const std::vector<double> ainv = {5.8125, -2.625, -0.3125, nan, 1.25, 0.125, nan, nan, 0.0625};
    // unit: [1 . .; 4 1 .; 2 -2 1]^-1 = [1 . .; -4 1 .; -10 2 1], the diagonal NaN throughout
    const std::vector<double> lu = {nan, 4, 2, nan, nan, -2, nan, nan, nan};
    const std::vector<double> xu = {nan, -4, -10, nan, nan, 2, nan, nan, nan};

    {  // DistMatrix, both triangles
        DM<double> A(3, 3, g);
        A.SetLocalBlock(l.data(), 3);
        El::TriangularInverse(El::LOWER, El::NON_UNIT, A);
        EXPECT(Same(Local(A), x));
        A.SetLocalBlock(Transposed(l).data(), 3);
        El::TriangularInverse(El::UPPER, El::NON_UNIT, A);
        EXPECT(Same(Local(A), Transposed(x)));
        A.SetLocalBlock(lu.data(), 3);
        El::TriangularInverse(El::LOWER, El::UNIT, A);
        EXPECT(Same(Local(A), xu));
        A.SetLocalBlock(Transposed(lu).data(), 3);
        El::TriangularInverse(El::UPPER, El::UNIT, A);
        EXPECT(Same(Local(A), Transposed(xu)));

        A.SetLocalBlock(l.data(), 3);
        El::Trtrmm(El::LOWER, A);
        EXPECT(Same(Local(A), ltl));
        A.SetLocalBlock(Transposed(l).data(), 3);
        El::Trtrmm(El::UPPER, A, true);  // U U^T with U = L^T; conjugation is the identity
        EXPECT(Same(Local(A), Transposed(ltl)));

        A.SetLocalBlock(a.data(), 3);
        El::HPDInverse(El::LOWER, A);
        EXPECT(Same(Local(A), ainv));
        A.SetLocalBlock(Transposed(a).data(), 3);
        El::HPDInverse(El::UPPER, A);
        EXPECT(Same(Local(A), Transposed(ainv)));

        DM<double> R(3, 2, g);
        int threw = 0;
        try { El::TriangularInverse(El::LOWER, El::NON_UNIT, R); }
        catch (const El::LogicError&) { ++threw; }
        try { El::Trtrmm(El::LOWER, R); }
        catch (const El::LogicError&) { ++threw; }
        try { El::HPDInverse(El::LOWER, R); }
        catch (const El::LogicError&) { ++threw; }
        EXPECT(threw == 3);  // A must be square
    }
    {  // a distribution other than [MC,MR] goes through the proxy
        DM<double, El::VC, El::STAR> A(3, 3, g);
        A.SetLocalBlock(a.data(), 3);
        El::HPDInverse(El::LOWER, A);
        EXPECT(Same(Local(A), ainv));
    }
    {  // the local forms on a [*,*] matrix
        DM<double, El::STAR, El::STAR> A(3, 3, g);
        A.SetLocalBlock(l.data(), 3);
        El::LocalTriangularInverse(El::LOWER, El::NON_UNIT, A);
        EXPECT(Same(Local(A), x));
        A.SetLocalBlock(a.data(), 3);
        El::LocalHPDInverse(El::LOWER, A);
        EXPECT(Same(Local(A), ainv));
    }
    {  // Matrix
        El::Matrix<double, kDev> A(3, 3);
        auto set = [&](const std::vector<double>& v) {
            for (Int j = 0; j < 3; ++j)
                for (Int i = 0; i < 3; ++i) A.Set(i, j, v[i + 3 * j]);
        };
        auto same = [&](const std::vector<double>& v) {
            bool ok = true;
            for (Int j = 0; j < 3; ++j)
                for (Int i = 0; i < 3; ++i)
                    ok = ok && (std::isnan(v[i + 3 * j]) ? std::isnan(A.Get(i, j)) : A.Get(i, j) == v[i + 3 * j]);
            return ok;
        };
        set(l);
        El::TriangularInverse(El::LOWER, El::NON_UNIT, A);
        EXPECT(same(x));
        set(l);
        El::Trtrmm(El::LOWER, A);
        EXPECT(same(ltl));
        set(Transposed(a));
        El::HPDInverse(El::UPPER, A);
        EXPECT(same(Transposed(ainv)));
        El::Matrix<double, kDev> R(3, 2);
        bool threw = false;
        try { El::HPDInverse(El::LOWER, R); }
        catch (const El::LogicError&) { threw = true; }
        EXPECT(threw);
    }
    {  // not HPD: the second pivot is 16 - 4^2 = 0
        DM<double> A(3, 3, g);
        std::vector<double> bad = a;
        bad[4] = 16;
        A.SetLocalBlock(bad.data(), 3);
        int column = 0;
        try { El::HPDInverse(El::LOWER, A); }
        catch (const El::NonHPDMatrixException& e) { column = e.Column(); }
        EXPECT(column == 2);
        // and the library is still usable
        A.SetLocalBlock(a.data(), 3);
        El::HPDInverse(El::LOWER, A);
        EXPECT(Same(Local(A), ainv));
    }
    El::Finalize();
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("El::HPDInverse API test OK\n");
    return 0;
}
