// El::Gemv / LocalGemv / Ger / Geru / Symv / Hemv / symv::LocalColAccumulate / Syr /
// Her / Syr2 / Her2 through the drop-in header (include/El.hpp), on Matrix and on
// DistMatrix over a 1x1 grid, Device::CPU (or Device::GPU with -DEL_TEST_GPU), each
// against a hand-computed answer on
//   A = [1 2; 3 4; 5 6] (3 x 2),  S = [2 -1 0; -1 2 -1; 0 -1 2] given by one triangle.
#include <El.hpp>

#include <cmath>
#include <cstdio>
#include <vector>

#ifdef EL_TEST_GPU
constexpr El::Device kDev = El::Device::GPU;
#else
constexpr El::Device kDev = El::Device::CPU;
#endif
template <typename T, El::Dist U = El::MC, El::Dist V = El::MR>
using DM = El::DistMatrix<T, U, V, El::ELEMENT, kDev>;
using Mat = El::Matrix<double, kDev>;
using Vec = std::vector<double>;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

template <typename M>
static Vec Local(const M& A) {
    Vec h(A.LocalHeight() * A.LocalWidth());
    if (!h.empty()) A.GetLocalBlock(h.data(), A.LocalHeight());
    return h;
}
template <typename M>
static void Put(M& A, const Vec& v) { A.SetLocalBlock(v.data(), A.LocalHeight()); }

static Mat Make(El::Int m, El::Int n, const Vec& v) {
    Mat A(m, n);
    for (El::Int j = 0; j < n; ++j)
        for (El::Int i = 0; i < m; ++i) A.Set(i, j, v[i + m * j]);
    return A;
}
static Vec Values(const Mat& A) {
    Vec v;
    for (El::Int j = 0; j < A.Width(); ++j)
        for (El::Int i = 0; i < A.Height(); ++i) v.push_back(A.Get(i, j));
    return v;
}

int main() {
    El::Initialize();
    El::Grid g;  // 1x1 over COMM_SELF
    const double nan = std::nan("");
    const Vec a = {1, 3, 5, 2, 4, 6};                           // column-major 3 x 2
    const Vec sl = {2, -1, 0, nan, 2, -1, nan, nan, 2};         // lower triangle, the rest poisoned
    const Vec su = {2, nan, nan, -1, 2, nan, 0, -1, 2};         // upper triangle
    const Vec x2 = {1, -1}, x3 = {1, 2, 3}, y3 = {1, 1, 1}, w3 = {1, 0, -1};

    {  // Matrix
        Mat A = Make(3, 2, a), x = Make(2, 1, x2), y = Make(3, 1, y3), xr = Make(1, 3, x3), z;
        El::Gemv(El::NORMAL, 2.0, A, x, 3.0, y);  // 2 (A x) + 3 y = 2 (-1,-1,-1) + 3
        EXPECT(Values(y) == (Vec{1, 1, 1}));
        El::Gemv(El::TRANSPOSE, 1.0, A, xr, z);   // A^T (1,2,3) with x a row vector; z resized
        EXPECT(z.Height() == 2 && z.Width() == 1 && Values(z) == (Vec{22, 28}));
        El::Gemv(El::ADJOINT, 1.0, A, xr, 0.0, z);
        EXPECT(Values(z) == (Vec{22, 28}));
        El::Ger(1.0, Make(3, 1, x3), x, A);       // A += (1,2,3) (1,-1)^T
        EXPECT(Values(A) == (Vec{2, 5, 8, 1, 2, 3}));
        El::Geru(-1.0, Make(3, 1, x3), x, A);
        EXPECT(Values(A) == a);

        Mat L = Make(3, 3, sl), U = Make(3, 3, su), v = Make(3, 1, x3), r = Make(3, 1, y3);
        El::Symv(El::LOWER, 1.0, L, v, 1.0, r);   // S (1,2,3) + 1 = (0,0,4) + 1
        EXPECT(Values(r) == (Vec{1, 1, 5}));
        El::Hemv(El::UPPER, 1.0, U, v, 0.0, r);
        EXPECT(Values(r) == (Vec{0, 0, 4}));
        El::Syr(El::LOWER, 1.0, v, L);            // + (1,2,3)(1,2,3)^T on the lower triangle
        {
            const Vec got = Values(L);
            EXPECT(got[0] == 3 && got[1] == 1 && got[2] == 3 && got[4] == 6 && got[5] == 5 && got[8] == 11);
            EXPECT(std::isnan(got[3]) && std::isnan(got[6]) && std::isnan(got[7]));
        }
        El::Her(El::LOWER, -1.0, v, L);
        El::Syr2(El::UPPER, 1.0, v, Make(3, 1, w3), U);  // + x w^T + w x^T
        {
            const Vec got = Values(U);  // x w^T + w x^T = [2 2 2; 2 0 -2; 2 -2 -6]
            EXPECT(got[0] == 4 && got[3] == 1 && got[4] == 2 && got[6] == 2 && got[7] == -3 && got[8] == -4);
            EXPECT(std::isnan(got[1]) && std::isnan(got[2]) && std::isnan(got[5]));
        }
        El::Her2(El::UPPER, -1.0, v, Make(3, 1, w3), U);
        EXPECT(Values(U)[0] == 2 && Values(U)[7] == -1);
        bool threw = false;
        try { El::Gemv(El::NORMAL, 1.0, A, v, 0.0, y); }
        catch (const El::LogicError&) { threw = true; }
        EXPECT(threw);  // x has 3 entries, A 2 columns
    }
    {  // DistMatrix
        DM<double> A(3, 2, g), x(2, 1, g), y(3, 1, g), xr(1, 3, g), z(1, 1, g);
        Put(A, a); Put(x, x2); Put(y, y3); Put(xr, x3);
        El::Gemv(El::NORMAL, 2.0, A, x, 3.0, y);
        EXPECT(Local(y) == (Vec{1, 1, 1}));
        El::Gemv(El::TRANSPOSE, 1.0, A, xr, z);
        EXPECT(z.Height() == 2 && z.Width() == 1 && Local(z) == (Vec{22, 28}));
        DM<double> yr(1, 2, g);  // y as a row vector
        Put(yr, Vec{1, 1});
        El::Gemv(El::ADJOINT, 1.0, A, xr, -1.0, yr);
        EXPECT(Local(yr) == (Vec{21, 27}));
        DM<double> c3(3, 1, g);
        Put(c3, x3);
        El::Ger(1.0, c3, x, A);
        EXPECT(Local(A) == (Vec{2, 5, 8, 1, 2, 3}));
        El::Geru(-1.0, c3, x, A);
        EXPECT(Local(A) == a);

        DM<double, El::MR, El::STAR> x_mr(2, 1, g);
        DM<double, El::MC, El::STAR> y_mc(3, 1, g);
        Put(x_mr, x2); Put(y_mc, y3);
        El::LocalGemv(El::NORMAL, 1.0, A, x_mr, 1.0, y_mc);
        EXPECT(Local(y_mc) == (Vec{0, 0, 0}));

        DM<double> L(3, 3, g), U(3, 3, g), r(3, 1, g), w(3, 1, g);
        Put(L, sl); Put(U, su); Put(r, y3); Put(w, w3);
        El::Symv(El::LOWER, 1.0, L, c3, 1.0, r);
        EXPECT(Local(r) == (Vec{1, 1, 5}));
        El::Hemv(El::UPPER, 1.0, U, xr, 0.0, r);  // x as a row vector
        EXPECT(Local(r) == (Vec{0, 0, 4}));
        DM<double, El::MC, El::STAR> x_mc(3, 1, g), z_mc(3, 1, g);
        DM<double, El::MR, El::STAR> x_mr3(3, 1, g), z_mr(3, 1, g);
        Put(x_mc, x3); Put(x_mr3, x3);
        El::Zero(z_mc); El::Zero(z_mr);
        El::symv::LocalColAccumulate(El::LOWER, 1.0, L, x_mc, x_mr3, z_mc, z_mr);
        // tril(S) x = (2, 3, 4); strict tril(S)^T x = (-2, -3, 0); the sum is S x
        EXPECT(Local(z_mc) == (Vec{2, 3, 4}) && Local(z_mr) == (Vec{-2, -3, 0}));
        El::Syr(El::LOWER, 1.0, c3, L);
        {
            const Vec got = Local(L);
            EXPECT(got[0] == 3 && got[1] == 1 && got[2] == 3 && got[4] == 6 && got[5] == 5 && got[8] == 11);
            EXPECT(std::isnan(got[3]) && std::isnan(got[6]) && std::isnan(got[7]));
        }
        El::Her(El::LOWER, -1.0, c3, L);
        EXPECT(Local(L)[0] == 2 && Local(L)[5] == -1);
        El::Syr2(El::UPPER, 1.0, c3, w, U);
        {
            const Vec got = Local(U);
            EXPECT(got[0] == 4 && got[3] == 1 && got[4] == 2 && got[6] == 2 && got[7] == -3 && got[8] == -4);
            EXPECT(std::isnan(got[1]) && std::isnan(got[2]) && std::isnan(got[5]));
        }
        El::Her2(El::UPPER, -1.0, c3, w, U);
        EXPECT(Local(U)[0] == 2 && Local(U)[7] == -1);

        bool threw = false;
        try { El::Symv(El::LOWER, 1.0, A, x, 0.0, y); }
        catch (const El::LogicError&) { threw = true; }
        EXPECT(threw);  // A is not square
        DM<float> H(3, 3, g);
        DM<float> hv(3, 1, g);
        El::Fill(H, 1.0f);
        El::Fill(hv, 1.0f);
        El::Syr(El::LOWER, 2.0f, hv, H);
        EXPECT(H.Get(2, 0) == 3.0f && H.Get(0, 2) == 1.0f);
    }
    El::Finalize();
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("El Level-2 API test OK\n");
    return 0;
}
