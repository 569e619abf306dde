// The Strassen-Winograd schedule of strassen.hpp.
//
// With op(A) = [A11 A12; A21 A22], op(B) and C cut likewise into halves:
//   S1 = A21 + A22   S2 = S1 - A11   S3 = A11 - A21   S4 = A12 - S2
//   T1 = B12 - B11   T2 = B22 - T1   T3 = B22 - B12   T4 = T2 - B21
//   P1 = A11 B11  P2 = A12 B21  P3 = S4 B22  P4 = A22 T4  P5 = S1 T1  P6 = S2 T2  P7 = S3 T3
//   C11 = P1 + P2            C12 = P1 + P6 + P5 + P3
//   C21 = P1 + P6 + P7 - P4  C22 = P1 + P6 + P7 + P5
// Three temporaries: S and T (the operand sums, in the stored layout of A's and
// B's quadrants, so ta / tb reach the kernel unchanged) and M, which collects
// U2 = P1 + P6 and U3 = U2 + P7 through the GEMM's own beta = 1.  P2, P3 and P4
// feed one quadrant each and go straight into it.  beta is applied at the first
// write of each quadrant; with beta = 0 no quadrant of C is read before it has
// been written.  Per element of a quadrant the additions move 4 x 6 (sums) + 5
// + 3 + 3 + 5 (scatters) = 40 elements.  A sub-product that passes the inner
// threshold (Knobs::min2) runs the same schedule one level down, with S, T and M
// of its own.
#include "strassen.hpp"
#include "exec.hpp"
#include <cstdlib>

namespace elx {
namespace strassen {

Knobs ReadKnobs() {
    Knobs kn{2, kDefaultMin, kDefaultMin2, false};
    const char* lv = getenv("ELX_GEMM_STRASSEN");
    if (lv) kn.levels = std::max(0, std::min(2, atoi(lv)));
    if (const char* v = getenv("ELX_GEMM_STRASSEN_MIN")) {
        kn.min = std::max<Int>(2, atoll(v));
        kn.forced = true;
        if (lv) kn.min2 = kn.min;  // two levels asked for by name: both under the one threshold
    }
    if (const char* v = getenv("ELX_GEMM_STRASSEN_MIN2")) kn.min2 = std::max<Int>(2, atoll(v));
    return kn;
}

bool Eligible(Device dev, DType t, Int m, Int n, Int k, double alpha, const Knobs& kn) {
    if (t != DType::F64 && t != DType::F32) return false;
    if (dev != Device::GPU && !kn.forced) return false;
    if ((m | n | k) & 1) return false;
    return std::min(m, std::min(n, k)) >= kn.min && alpha != 0.0;
}

namespace {

// one temporary: kern::workspace_alloc on the GPU (stream-ordered, no throw), the heap on the host
struct Work {
    Device dev;
    hipStream_t s;
    void* p = nullptr;
    Work(Device d, hipStream_t st) : dev(d), s(st) {}
    Work(const Work&) = delete;
    Work& operator=(const Work&) = delete;
    bool Alloc(size_t bytes) {
        if (dev == Device::GPU) return kern::workspace_alloc(&p, bytes, s) == hipSuccess && p != nullptr;
        p = std::malloc(bytes);
        return p != nullptr;
    }
    ~Work() {
        if (!p) return;
        if (dev == Device::GPU) (void)kern::workspace_free(p, s);
        else std::free(p);
    }
};

// a sub-product: another level where levels remain and it is eligible under the
// inner threshold, else the plain kernel
int Multiply(int levels, const Knobs& kn, Device dev, DType t, bool ta, bool tb, Int m, Int n, Int k, double alpha,
             const void* A, Int lda, const void* B, Int ldb, double beta, void* C, Int ldc, hipStream_t s) {
    Knobs inner = kn;
    inner.min = kn.min2;
    const int used = Gemm(levels, inner, dev, t, ta, tb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, s);
    if (used == 0) exec::GemmPlain(dev, t, ta, tb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, s);
    return used;
}

}  // namespace

int Gemm(int levels, const Knobs& kn, Device dev, DType t, bool ta, bool tb, Int m, Int n, Int k, double alpha,
         const void* A, Int lda, const void* B, Int ldb, double beta, void* C, Int ldc, hipStream_t s) {
    if (levels <= 0 || !Eligible(dev, t, m, n, k, alpha, kn)) return 0;
    const Int m2 = m / 2, n2 = n / 2, k2 = k / 2;
    const size_t es = DTypeSize(t);
    // stored shapes of a quadrant of A and of B
    const Int ra = ta ? k2 : m2, ca = ta ? m2 : k2, rb = tb ? n2 : k2, cb = tb ? k2 : n2;
    Work Sw(dev, s), Tw(dev, s), Mw(dev, s);
    if (!Sw.Alloc((size_t)ra * ca * es) || !Tw.Alloc((size_t)rb * cb * es) || !Mw.Alloc((size_t)m2 * n2 * es)) return 0;
    void* S = Sw.p;
    void* T = Tw.p;
    void* M = Mw.p;

    const char* a = static_cast<const char*>(A);
    const char* b = static_cast<const char*>(B);
    char* c = static_cast<char*>(C);
    // quadrant (p, q) of op(A), op(B) and C as a view of the stored matrix
    auto Aq = [&](int p, int q) -> const void* { return a + (ta ? q * k2 + p * m2 * lda : p * m2 + q * k2 * lda) * (Int)es; };
    auto Bq = [&](int p, int q) -> const void* { return b + (tb ? q * n2 + p * k2 * ldb : p * k2 + q * n2 * ldb) * (Int)es; };
    auto Cq = [&](int p, int q) -> void* { return c + (p * m2 + q * n2 * ldc) * (Int)es; };

    // S := X + sx Y and T := V + sv W in one launch
    auto sums = [&](const void* X, Int ldx, const void* Y, Int ldy, double sx, const void* V, Int ldv, const void* W,
                    Int ldw, double sv) {
        const kern::QuadSum q[2] = {{ra, ca, S, ra, X, ldx, Y, ldy, sx}, {rb, cb, T, rb, V, ldv, W, ldw, sv}};
        exec::QuadSum(dev, t, q, 2, s);
    };
    auto scatter = [&](int nt, void* c0, double beta0, void* c1, double beta1) {
        const kern::QuadScatter q{m2, n2, M, m2, nt, {c0, c1}, {ldc, ldc}, {beta0, beta1}, {alpha, alpha}};
        exec::QuadScatter(dev, t, q, s);
    };
    int deep = 0;
    auto mul = [&](double al, const void* X, Int ldx, const void* Y, Int ldy, double be, void* Z, Int ldz) {
        deep = std::max(deep, Multiply(levels - 1, kn, dev, t, ta, tb, m2, n2, k2, al, X, ldx, Y, ldy, be, Z, ldz, s));
    };

    sums(Aq(1, 0), lda, Aq(1, 1), lda, 1.0, Bq(0, 1), ldb, Bq(0, 0), ldb, -1.0);  // S1, T1
    mul(1.0, S, ra, T, rb, 0.0, M, m2);                                           // P5
    scatter(2, Cq(0, 1), beta, Cq(1, 1), beta);                                   // C12, C22 = beta C + alpha P5
    sums(S, ra, Aq(0, 0), lda, -1.0, Bq(1, 1), ldb, T, rb, -1.0);                 // S2, T2
    mul(1.0, Aq(0, 0), lda, Bq(0, 0), ldb, 0.0, M, m2);                           // P1
    scatter(1, Cq(0, 0), beta, nullptr, 0.0);                                     // C11 = beta C11 + alpha P1
    mul(alpha, Aq(0, 1), lda, Bq(1, 0), ldb, 1.0, Cq(0, 0), ldc);                 // C11 += alpha P2
    mul(1.0, S, ra, T, rb, 1.0, M, m2);                                           // U2 = P1 + P6
    sums(Aq(0, 1), lda, S, ra, -1.0, T, rb, Bq(1, 0), ldb, -1.0);                 // S4, T4
    mul(alpha, S, ra, Bq(1, 1), ldb, 1.0, Cq(0, 1), ldc);                         // C12 += alpha P3
    mul(-alpha, Aq(1, 1), lda, T, rb, beta, Cq(1, 0), ldc);                       // C21 = beta C21 - alpha P4
    scatter(1, Cq(0, 1), 1.0, nullptr, 0.0);                                      // C12 += alpha U2
    sums(Aq(0, 0), lda, Aq(1, 0), lda, -1.0, Bq(1, 1), ldb, Bq(0, 1), ldb, -1.0);  // S3, T3
    mul(1.0, S, ra, T, rb, 1.0, M, m2);                                           // U3 = U2 + P7
    scatter(2, Cq(1, 0), 1.0, Cq(1, 1), 1.0);                                     // C21, C22 += alpha U3
    return 1 + deep;
}

}  // namespace strassen
}  // namespace elx
