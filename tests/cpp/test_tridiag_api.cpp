// El::HermitianTridiag / herm_tridiag::ApplyQ / ExplicitCondensed through the
// drop-in header (include/El.hpp) on Device::CPU matrices over a 1x1 grid, against
// a hand-computed 3 x 3 case:
//   A = [1 3 4; 3 2 1; 4 1 3], LOWER.  Column 0: alpha = 3, tail (4), beta = -5, t =
//   8/5, u = 1/2; H_0 = I - 1.6 [1; .5][1; .5]^T = [-.6 -.8; -.8 .6] on rows 1..2 and
//   H_0 [2 1; 1 3] H_0 = [3.6 -.2; -.2 1.4].  Column 1: alpha = -0.2 with an empty
//   tail: t = 2, beta = 0.2.  T = tridiag(diag 1, 3.6, 1.4; off -5, 0.2).
//   UPPER on J A J (J reverses the order) gives the same numbers reversed.
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
    const std::vector<double> a = {1, 3, 4, 3, 2, 1, 4, 1, 3};  // column-major
    const std::vector<double> lower = {1, -5, 0.5, 3, 3.6, 0.2, 4, 1, 1.4};
    const std::vector<double> ar = {3, 1, 4, 1, 2, 3, 4, 3, 1};  // J A J
    const std::vector<double> upper = {1.4, 1, 4, 0.2, 3.6, 3, 0.5, -5, 1};
    const std::vector<double> eye = {1, 0, 0, 0, 1, 0, 0, 0, 1};

    for (int pass = 0; pass < 2; ++pass) {
        const El::UpperOrLower uplo = pass == 0 ? El::LOWER : El::UPPER;
        const std::vector<double>& in = pass == 0 ? a : ar;
        DM<double> A(3, 3, g), t(1, 1, g), Q(3, 3, g);
        A.SetLocalBlock(in.data(), 3);
        El::HermitianTridiag(uplo, A, t);
        EXPECT(Near(Local(A), pass == 0 ? lower : upper));
        EXPECT(t.Height() == 2 && t.Width() == 1);
        EXPECT(Near(Local(t), pass == 0 ? std::vector<double>{1.6, 2} : std::vector<double>{2, 1.6}));

        // Q from the identity, then Q T Q^T = A and Q^T Q = I
        Q.SetLocalBlock(eye.data(), 3);
        El::herm_tridiag::ApplyQ(El::LEFT, uplo, El::NORMAL, A, t, Q);
        const std::vector<double> q = Local(Q);
        const double d[3] = {pass == 0 ? 1 : 1.4, 3.6, pass == 0 ? 1.4 : 1};
        const double e[2] = {pass == 0 ? -5 : 0.2, pass == 0 ? 0.2 : -5};
        std::vector<double> back(9, 0.0);
        for (Int i = 0; i < 3; ++i)
            for (Int j = 0; j < 3; ++j)
                for (Int k = 0; k < 3; ++k) {
                    back[i + 3 * j] += q[i + 3 * k] * d[k] * q[j + 3 * k];
                    if (k < 2) back[i + 3 * j] += e[k] * (q[i + 3 * k] * q[j + 3 * (k + 1)] + q[i + 3 * (k + 1)] * q[j + 3 * k]);
                }
        EXPECT(Near(back, in));
        El::herm_tridiag::ApplyQ(El::LEFT, uplo, El::ADJOINT, A, t, Q);
        EXPECT(Near(Local(Q), eye));

        bool threw = false;
        try { El::herm_tridiag::ApplyQ(El::RIGHT, uplo, El::NORMAL, A, t, Q); }
        catch (const El::LogicError&) { threw = true; }
        EXPECT(threw);  // only LEFT

        DM<double> C(3, 3, g);
        C.SetLocalBlock(in.data(), 3);
        El::herm_tridiag::ExplicitCondensed(uplo, C);
        std::vector<double> want = pass == 0 ? lower : upper;
        want[pass == 0 ? 2 : 6] = 0;  // the one reflector entry
        EXPECT(Near(Local(C), want));

        threw = false;
        DM<double> Rect(3, 2, g);
        try { El::HermitianTridiag(uplo, Rect, t); }
        catch (const El::LogicError&) { threw = true; }
        EXPECT(threw);  // not square
    }
    {  // Matrix
        El::Matrix<double, kDev> A(3, 3), t;
        for (Int j = 0; j < 3; ++j)
            for (Int i = 0; i < 3; ++i) A.Set(i, j, a[i + 3 * j]);
        El::HermitianTridiag(El::LOWER, A, t);
        EXPECT(t.Height() == 2 && t.Width() == 1);
        for (Int j = 0; j < 3; ++j)
            for (Int i = 0; i < 3; ++i) EXPECT(std::fabs(A.Get(i, j) - lower[i + 3 * j]) <= 1e-14);
        EXPECT(std::fabs(t.Get(0, 0) - 1.6) <= 1e-15 && t.Get(1, 0) == 2);
    }
    El::Finalize();
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("El::HermitianTridiag API test OK\n");
    return 0;
}
