// El::QR / qr::ApplyQ / SolveAfter / Explicit / ExplicitTriang / LeastSquares through
// the drop-in header (include/El.hpp) on Device::CPU matrices over a 1x1 grid,
// against a hand-computed 3 x 2 case:
//   A = [3 1; 4 2; 0 2].  Column 0: alpha = 3, nu = 4, beta = -5, t = 8/5, u = (1/2, 0),
//   d = -1; z = 1 + 2/2 = 2, so column 1 becomes (1 - 16/5, 2 - 8/5, 2) = (-2.2, 0.4, 2)
//   and row 0 of R is (5, 2.2).  Column 1: alpha = 0.4, nu = 2, beta = -sqrt(4.16),
//   t = (beta - 0.4) / beta, u = 2 / (0.4 - beta), d = -1.
//   R = [5 2.2; 0 sqrt(4.16)],  A [1; 2] = [5; 8; 4].
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
    if (!h.empty()) A.GetLocalBlock(h.data(), A.LocalHeight());
    return h;
}

static bool Near(const std::vector<double>& a, const std::vector<double>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (!(std::fabs(a[i] - b[i]) <= 1e-14)) return false;
    return true;
}

int main() {
    using El::Int;
    El::Initialize();
    El::Grid g;  // 1x1 over COMM_SELF
    const std::vector<double> a = {3, 4, 0, 1, 2, 2};  // column-major
    const double r11 = std::sqrt(4.16), t1 = (-r11 - 0.4) / -r11, u1 = 2 / (0.4 + r11);
    const std::vector<double> packed = {5, 0.5, 0, 2.2, r11, u1};
    const std::vector<double> rfull = {5, 0, 2.2, r11};
    const std::vector<double> b = {5, 8, 4};

    {  // DistMatrix: the factors, ApplyQ, the solves
        DM<double> A(3, 2, g), t(1, 1, g), d(1, 1, g), B(3, 1, g), X(1, 1, g);
        A.SetLocalBlock(a.data(), 3);
        El::QR(A, t, d);
        EXPECT(Near(Local(A), packed));
        EXPECT(t.Height() == 2 && t.Width() == 1 && d.Height() == 2 && d.Width() == 1);
        EXPECT(Near(Local(t), {8.0 / 5.0, t1}));
        EXPECT(Local(d) == (std::vector<double>{-1, -1}));

        // Q^T b = [R [1; 2]; 0] and back
        B.SetLocalBlock(b.data(), 3);
        El::qr::ApplyQ(El::LEFT, El::ADJOINT, A, t, d, B);
        EXPECT(Near(Local(B), {5 + 2 * 2.2, 2 * r11, 0}));
        El::qr::ApplyQ(El::LEFT, El::NORMAL, A, t, d, B);
        EXPECT(Near(Local(B), b));

        B.SetLocalBlock(b.data(), 3);
        El::qr::SolveAfter(El::NORMAL, A, t, d, B, X);
        EXPECT(X.Height() == 2 && X.Width() == 1 && Near(Local(X), {1, 2}));
        // minimum norm: A^T x = c with x in range(A); x = A y, A^T A y = c.  c = A^T b
        DM<double> C(2, 1, g);
        const std::vector<double> c = {3 * 5 + 4 * 8, 5 + 16 + 8};
        C.SetLocalBlock(c.data(), 2);
        El::qr::SolveAfter(El::ADJOINT, A, t, d, C, X);
        EXPECT(X.Height() == 3 && Near(Local(X), b));

        bool threw = false;
        try { El::qr::ApplyQ(El::RIGHT, El::NORMAL, A, t, d, B); }
        catch (const El::LogicError&) { threw = true; }
        EXPECT(threw);  // only LEFT
        threw = false;
        try { El::qr::SolveAfter(El::NORMAL, A, t, d, C, X); }
        catch (const El::LogicError&) { threw = true; }
        EXPECT(threw);  // A and B do not conform
    }
    {  // Explicit, ExplicitTriang, LeastSquares (A is left as it was)
        DM<double> A(3, 2, g), R(1, 1, g), B(3, 1, g), X(1, 1, g);
        A.SetLocalBlock(a.data(), 3);
        B.SetLocalBlock(b.data(), 3);
        El::LeastSquares(El::NORMAL, A, B, X);
        EXPECT(Near(Local(X), {1, 2}));
        EXPECT(Local(A) == a);
        El::qr::Explicit(A, R);
        EXPECT(A.Height() == 3 && A.Width() == 2 && R.Height() == 2 && R.Width() == 2);
        EXPECT(Near(Local(R), rfull));
        // Q = A R^-1: columns (3, 4, 0) / 5 and ((1, 2, 2) - 2.2 q0) / r11
        EXPECT(Near(Local(A), {0.6, 0.8, 0, (1 - 2.2 * 0.6) / r11, (2 - 2.2 * 0.8) / r11, 2 / r11}));
        A.SetLocalBlock(a.data(), 3);
        El::qr::ExplicitTriang(A);
        EXPECT(A.Height() == 2 && A.Width() == 2 && Near(Local(A), rfull));
        DM<double> Wd(2, 3, g);
        bool threw = false;
        try { El::LeastSquares(El::NORMAL, Wd, B, X); }
        catch (const El::UnsupportedError&) { threw = true; }
        EXPECT(threw);  // m < n
    }
    {  // Matrix
        El::Matrix<double, kDev> A(3, 2), t, d;
        for (Int j = 0; j < 2; ++j)
            for (Int i = 0; i < 3; ++i) A.Set(i, j, a[i + 3 * j]);
        El::QR(A, t, d);
        EXPECT(t.Height() == 2 && t.Width() == 1 && d.Height() == 2);
        for (Int j = 0; j < 2; ++j)
            for (Int i = 0; i < 3; ++i) EXPECT(std::fabs(A.Get(i, j) - packed[i + 3 * j]) <= 1e-14);
        EXPECT(std::fabs(t.Get(0, 0) - 1.6) <= 1e-15 && d.Get(0, 0) == -1 && d.Get(1, 0) == -1);
    }
    El::Finalize();
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("El::QR API test OK\n");
    return 0;
}
