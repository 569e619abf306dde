#include <cstdlib>
#include "exec.hpp"
#include "../kernels/elem.hpp"
#include <cmath>
#include <vector>

namespace elx {
namespace exec {

namespace {

// Host element access in the compute type of each dtype (f16/bf16 -> float).
template <typename S> struct H;
template <> struct H<double> {
    using C = double;
    static C ld(const double* p) { return *p; }
    static void st(double* p, C v) { *p = v; }
};
template <> struct H<float> {
    using C = float;
    static C ld(const float* p) { return *p; }
    static void st(float* p, C v) { *p = v; }
};
struct Half16 { uint16_t b; };
struct Brain16 { uint16_t b; };
template <> struct H<Half16> {
    using C = float;
    static C ld(const Half16* p) { return HalfToFloat(p->b); }
    static void st(Half16* p, C v) { p->b = FloatToHalf(v); }
};
template <> struct H<Brain16> {
    using C = float;
    static C ld(const Brain16* p) { return BF16ToFloat(p->b); }
    static void st(Brain16* p, C v) { p->b = FloatToBF16(v); }
};

#define HOST_DTYPE_SWITCH(t, S, ...)                                   \
    switch (t) {                                                       \
    case DType::F64: { using S = double; __VA_ARGS__; break; }         \
    case DType::F32: { using S = float; __VA_ARGS__; break; }          \
    case DType::F16: { using S = Half16; __VA_ARGS__; break; }         \
    case DType::BF16: { using S = Brain16; __VA_ARGS__; break; }       \
    default: throw LogicError(Cat("dtype ", DTypeName(t), " is not a matrix type")); \
    }

template <typename S>
void cpu_copy(const Copy2D& d, bool axpy, double alpha) {
    const S* src = static_cast<const S*>(d.src);
    S* dst = static_cast<S*>(d.dst);
    using C = typename H<S>::C;
    const C a = (C)alpha;
    for (Int j = 0; j < d.n; ++j)
        for (Int i = 0; i < d.m; ++i) {
            const S* x = src + i * d.scs + j * d.srs;
            S* y = dst + i * d.dcs + j * d.drs;
            if (axpy) H<S>::st(y, H<S>::ld(y) + a * H<S>::ld(x));
            else *y = *x;
        }
}

template <typename S>
void cpu_gemm(bool ta, bool tb, Int m, Int n, Int k, double alpha, const S* A, Int lda, const S* B,
              Int ldb, double beta, S* C, Int ldc) {
    using Cm = typename H<S>::C;
    std::vector<Cm> acc(static_cast<size_t>(m));
    for (Int j = 0; j < n; ++j) {
        std::fill(acc.begin(), acc.end(), Cm(0));
        for (Int l = 0; l < k; ++l) {
            const Cm b = H<S>::ld(tb ? B + j + l * ldb : B + l + j * ldb);
            if (b == Cm(0)) continue;
            if (!ta) {
                const S* acol = A + l * lda;
                for (Int i = 0; i < m; ++i) acc[i] += H<S>::ld(acol + i) * b;
            } else {
                for (Int i = 0; i < m; ++i) acc[i] += H<S>::ld(A + l + i * lda) * b;
            }
        }
        for (Int i = 0; i < m; ++i) {
            S* c = C + i + j * ldc;
            const Cm v = (Cm)alpha * acc[i];
            H<S>::st(c, beta == 0.0 ? v : v + (Cm)beta * H<S>::ld(c));
        }
    }
}

template <typename Cm>
Cm cpu_map(int fn, Cm x) {
    switch (fn) {
    case ELX_MAP_IDENTITY: return x;
    case ELX_MAP_NEGATE: return -x;
    case ELX_MAP_ABS: return std::fabs(x);
    case ELX_MAP_SQUARE: return x * x;
    case ELX_MAP_SQRT: return std::sqrt(x);
    case ELX_MAP_EXP: return std::exp(x);
    case ELX_MAP_LOG: return std::log(x);
    case ELX_MAP_RELU: return x > Cm(0) ? x : Cm(0);
    case ELX_MAP_SIGMOID: return Cm(1) / (Cm(1) + std::exp(-x));
    case ELX_MAP_RECIP: return Cm(1) / x;
    case ELX_MAP_TANH: return std::tanh(x);
    default: throw LogicError(Cat("unknown entrywise functor ", fn));
    }
}

void check(hipError_t e, const char* what) {
    if (e != hipSuccess)
        throw HIPError(Cat(what, ": ", hipGetErrorName(e), " (", hipGetErrorString(e), ")"));
}

}  // namespace

// Pack / unpack launches on the comm stream run beside full-machine MFMA
// updates, so they are capped at ELX_COMM_COPY_WGS workgroups (default 256, one
// per CU): uncapped launches of thousands of workgroups at the comm stream's
// priority slowed the MFMA updates by 5-10 %, caps of 256-512 by 0-2 %
// (profiles/r02_comm_copy_cap.log; 0 = uncapped)
int CommCopyWGs() {
    static const int v = [] { const char* e = getenv("ELX_COMM_COPY_WGS"); return e ? atoi(e) : 256; }();
    return v;
}

void Copy2DBatch(Device dev, DType t, const Copy2D* d, int nd, bool axpy, double alpha, hipStream_t s) {
    if (nd <= 0) return;
    if (dev == Device::GPU) {
        const int cap = s != nullptr && s == Runtime::Get().CommStream() ? CommCopyWGs() : 0;
        check(kern::copy2d_batch(static_cast<int>(t), d, nd, axpy, alpha, s, cap), "copy2d_batch");
        return;
    }
    for (int q = 0; q < nd; ++q) HOST_DTYPE_SWITCH(t, S, cpu_copy<S>(d[q], axpy, alpha));
}

void ContractSum(Device dev, DType t, Int m, Int n, void* dst, Int dcs, Int drs, const ContractSource* src,
                 int nsrc, double alpha, hipStream_t s) {
    if (m <= 0 || n <= 0 || nsrc <= 0) return;
    if (dev == Device::GPU) {
        const int cap = s != nullptr && s == Runtime::Get().CommStream() ? CommCopyWGs() : 0;
        for (int q0 = 0; q0 < nsrc; q0 += kern::kMaxContractSources) {
            kern::ContractSum c{};
            c.m = m; c.n = n; c.dst = dst; c.dcs = dcs; c.drs = drs;
            c.nsrc = std::min(nsrc - q0, kern::kMaxContractSources);
            for (int q = 0; q < c.nsrc; ++q) {
                c.src[q] = src[q0 + q].p;
                c.scs[q] = src[q0 + q].cs;
                c.srs[q] = src[q0 + q].rs;
            }
            check(kern::contract_sum(static_cast<int>(t), c, alpha, s, cap), "contract_sum");
        }
        return;
    }
    // host: the same per-source axpys, in order
    for (int q = 0; q < nsrc; ++q) {
        const Copy2D d{m, n, src[q].p, src[q].cs, src[q].rs, dst, dcs, drs};
        HOST_DTYPE_SWITCH(t, S, cpu_copy<S>(d, true, alpha));
    }
}

namespace {
template <typename TS, typename TD>
void cpu_convert(const Copy2D& d) {
    using SS = typename kern::Elem<TS>::storage;
    using SD = typename kern::Elem<TD>::storage;
    const SS* src = static_cast<const SS*>(d.src);
    SD* dst = static_cast<SD*>(d.dst);
    for (Int j = 0; j < d.n; ++j)
        for (Int i = 0; i < d.m; ++i)
            dst[i * d.dcs + j * d.drs] = kern::convert_elem<TS, TD>(src[i * d.scs + j * d.srs]);
}
#define KERN_DTYPE_SWITCH(t, T, ...)                                     \
    switch (t) {                                                         \
    case DType::F64: { using T = double; __VA_ARGS__; break; }           \
    case DType::F32: { using T = float; __VA_ARGS__; break; }            \
    case DType::F16: { using T = kern::f16_t; __VA_ARGS__; break; }      \
    case DType::BF16: { using T = kern::bf16_t; __VA_ARGS__; break; }    \
    default: throw LogicError(Cat("dtype ", DTypeName(t), " is not a matrix type")); \
    }
}  // namespace

void Convert2D(Device dev, DType src_t, DType dst_t, const Copy2D& d, hipStream_t s) {
    if (d.m <= 0 || d.n <= 0) return;
    if (src_t == dst_t) { Copy2DBatch(dev, src_t, &d, 1, false, 0.0, s); return; }
    if (dev == Device::GPU) {
        check(kern::convert2d(static_cast<int>(src_t), static_cast<int>(dst_t), d, s), "convert2d");
        return;
    }
    KERN_DTYPE_SWITCH(src_t, TS, KERN_DTYPE_SWITCH(dst_t, TD, cpu_convert<TS, TD>(d)));
}

void Gemm(Device dev, DType t, bool ta, bool tb, Int m, Int n, Int k, double alpha, const void* A, Int lda,
          const void* B, Int ldb, double beta, void* C, Int ldc, hipStream_t s) {
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) {
        hipError_t e = hipSuccess;
        switch (t) {
        case DType::F64:
            e = kern::gemm_mfma<double>(ta, tb, m, n, k, alpha, static_cast<const double*>(A), lda,
                                        static_cast<const double*>(B), ldb, beta, static_cast<double*>(C), ldc, s);
            break;
        case DType::F32:
            e = kern::gemm_mfma<float>(ta, tb, m, n, k, (float)alpha, static_cast<const float*>(A), lda,
                                       static_cast<const float*>(B), ldb, (float)beta, static_cast<float*>(C),
                                       ldc, s);
            break;
        case DType::F16:
        case DType::BF16:
            e = kern::gemm_mfma_h(t == DType::BF16, ta, tb, m, n, k, (float)alpha,
                                  static_cast<const uint16_t*>(A), lda, static_cast<const uint16_t*>(B), ldb,
                                  (float)beta, static_cast<uint16_t*>(C), ldc, s);
            break;
        default:
            throw LogicError(Cat("dtype ", DTypeName(t), " is not a matrix type"));
        }
        check(e, "gemm_mfma");
        return;
    }
    HOST_DTYPE_SWITCH(t, S,
        cpu_gemm<S>(ta, tb, m, n, k, alpha, static_cast<const S*>(A), lda, static_cast<const S*>(B), ldb, beta,
                    static_cast<S*>(C), ldc));
}

void Fill(Device dev, DType t, Int m, Int n, double v, void* A, Int lda, hipStream_t s) {
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) { check(kern::fill2d((int)t, m, n, v, A, lda, s), "fill2d"); return; }
    HOST_DTYPE_SWITCH(t, S, {
        S* a = static_cast<S*>(A);
        for (Int j = 0; j < n; ++j)
            for (Int i = 0; i < m; ++i) H<S>::st(a + i + j * lda, (typename H<S>::C)v);
    });
}

void Scale(Device dev, DType t, Int m, Int n, double alpha, void* A, Int lda, hipStream_t s) {
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) { check(kern::scale2d((int)t, m, n, alpha, A, lda, s), "scale2d"); return; }
    HOST_DTYPE_SWITCH(t, S, {
        S* a = static_cast<S*>(A);
        using Cm = typename H<S>::C;
        for (Int j = 0; j < n; ++j)
            for (Int i = 0; i < m; ++i) H<S>::st(a + i + j * lda, (Cm)alpha * H<S>::ld(a + i + j * lda));
    });
}

namespace {
double NormMax(double a, double b) { return a != a ? a : b != b ? b : std::max(a, b); }
// mode 0: max |a|; mode 1: sum (a / scale)^2 — device partials reduced on the host
double NormReduce(Device dev, DType t, int mode, Int m, Int n, const void* A, Int lda, double scale, hipStream_t s) {
    double r = 0.0;
    if (m <= 0 || n <= 0) return r;
    if (dev == Device::GPU) {
        Buffer parts(Device::GPU, sizeof(double) * kern::kNormPartsMax, s);
        int np = 0;
        check(kern::norm_partials((int)t, mode, m, n, A, lda, scale, static_cast<double*>(parts.data()), &np, s),
              "norm_partials");
        std::vector<double> h(np);
        ELX_CHECK_HIP(hipMemcpyAsync(h.data(), parts.data(), sizeof(double) * np, hipMemcpyDeviceToHost, s));
        ELX_CHECK_HIP(hipStreamSynchronize(s));
        for (double v : h) r = mode == 0 ? NormMax(r, v) : r + v;
        return r;
    }
    HOST_DTYPE_SWITCH(t, S, {
        const S* a = static_cast<const S*>(A);
        for (Int j = 0; j < n; ++j)
            for (Int i = 0; i < m; ++i) {
                const double x = (double)H<S>::ld(a + i + j * lda);
                if (mode == 0) r = NormMax(r, std::fabs(x));
                else { const double y = x / scale; r += y * y; }
            }
    });
    return r;
}
}  // namespace

double AbsMax(Device dev, DType t, Int m, Int n, const void* A, Int lda, hipStream_t s) {
    return NormReduce(dev, t, 0, m, n, A, lda, 1.0, s);
}
double ScaledSumSq(Device dev, DType t, Int m, Int n, const void* A, Int lda, double scale, hipStream_t s) {
    return NormReduce(dev, t, 1, m, n, A, lda, scale, s);
}

void Hadamard(Device dev, DType t, Int m, Int n, const void* A, Int lda, const void* B, Int ldb, void* C,
              Int ldc, hipStream_t s) {
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) { check(kern::hadamard2d((int)t, m, n, A, lda, B, ldb, C, ldc, s), "hadamard2d"); return; }
    HOST_DTYPE_SWITCH(t, S, {
        const S* a = static_cast<const S*>(A);
        const S* b = static_cast<const S*>(B);
        S* c = static_cast<S*>(C);
        for (Int j = 0; j < n; ++j)
            for (Int i = 0; i < m; ++i)
                H<S>::st(c + i + j * ldc, H<S>::ld(a + i + j * lda) * H<S>::ld(b + i + j * ldb));
    });
}

void Map(Device dev, DType t, int fn, Int m, Int n, const void* A, Int lda, void* B, Int ldb, hipStream_t s) {
    if (fn < ELX_MAP_IDENTITY || fn > ELX_MAP_TANH) throw LogicError(Cat("unknown entrywise functor ", fn));
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) { check(kern::entrywise_map((int)t, fn, m, n, A, lda, B, ldb, s), "entrywise_map"); return; }
    HOST_DTYPE_SWITCH(t, S, {
        const S* a = static_cast<const S*>(A);
        S* b = static_cast<S*>(B);
        for (Int j = 0; j < n; ++j)
            for (Int i = 0; i < m; ++i) H<S>::st(b + i + j * ldb, cpu_map(fn, H<S>::ld(a + i + j * lda)));
    });
}

template <typename Cm>
Cm cpu_combine(int fn, Cm a, Cm b) {
    switch (fn) {
    case ELX_COMBINE_ADD: return a + b;
    case ELX_COMBINE_SUB: return b - a;
    case ELX_COMBINE_MUL: return a * b;
    case ELX_COMBINE_DIV: return b / a;
    case ELX_COMBINE_MAX: return a > b ? a : b;
    case ELX_COMBINE_MIN: return a < b ? a : b;
    case ELX_COMBINE_RELU_GRAD: return a > Cm(0) ? b : Cm(0);
    default: throw LogicError(Cat("unknown combine functor ", fn));
    }
}

void Combine(Device dev, DType t, int fn, Int m, Int n, const void* A, Int lda, void* B, Int ldb, hipStream_t s) {
    if (fn < ELX_COMBINE_ADD || fn > ELX_COMBINE_RELU_GRAD) throw LogicError(Cat("unknown combine functor ", fn));
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) { check(kern::combine((int)t, fn, m, n, A, lda, B, ldb, s), "combine"); return; }
    HOST_DTYPE_SWITCH(t, S, {
        const S* a = static_cast<const S*>(A);
        S* b = static_cast<S*>(B);
        for (Int j = 0; j < n; ++j)
            for (Int i = 0; i < m; ++i)
                H<S>::st(b + i + j * ldb, cpu_combine(fn, H<S>::ld(a + i + j * lda), H<S>::ld(b + i + j * ldb)));
    });
}

void Trapezoid(Device dev, DType t, bool lower, Int m, Int n, double alpha, const void* X, Int ldx, double beta,
               void* Y, Int ldy, Int i0, Int is, Int j0, Int js, Int offset, hipStream_t s) {
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) {
        check(kern::trapezoid2d((int)t, lower, m, n, alpha, X, ldx, beta, Y, ldy, i0, is, j0, js, offset, s),
              "trapezoid2d");
        return;
    }
    HOST_DTYPE_SWITCH(t, S, {
        using Cm = typename H<S>::C;
        const S* x = static_cast<const S*>(X);
        S* y = static_cast<S*>(Y);
        for (Int j = 0; j < n; ++j)
            for (Int i = 0; i < m; ++i) {
                const Int gi = i0 + i * is, gj = j0 + j * js - offset;
                if (lower ? gi < gj : gi > gj) continue;
                Cm v = (x && beta == 0.0) ? Cm(0) : (Cm)beta * H<S>::ld(y + i + j * ldy);
                if (x) v = v + (Cm)alpha * H<S>::ld(x + i + j * ldx);
                H<S>::st(y + i + j * ldy, v);
            }
    });
}

template <typename S>
void cpu_trsm(bool lower, bool trans, bool unit, Int m, Int n, const S* A, Int lda, S* B, Int ldb) {
    const bool forward = lower != trans;
    auto opA = [&](Int r, Int c) { return trans ? A[c + r * lda] : A[r + c * lda]; };
    for (Int j = 0; j < n; ++j) {
        S* x = B + j * ldb;
        for (Int s = 0; s < m; ++s) {
            const Int i = forward ? s : m - 1 - s;
            S xi = x[i];
            if (!unit) xi = xi / opA(i, i);
            x[i] = xi;
            if (forward)
                for (Int r = i + 1; r < m; ++r) x[r] = x[r] - opA(r, i) * xi;
            else
                for (Int r = 0; r < i; ++r) x[r] = x[r] - opA(r, i) * xi;
        }
    }
}

void Trsm(Device dev, DType t, bool lower, bool trans, bool unit, Int m, Int n, const void* A, Int lda, void* B,
          Int ldb, hipStream_t s) {
    if (t != DType::F64 && t != DType::F32) throw LogicError("Trsm: only float and double are supported");
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) {
        const size_t es = DTypeSize(t);
        if (m <= 256 && n >= 4 * m) {
            // many right-hand sides: W = op(A)^-1 (m lanes of substitution), then
            // B := W B as one MFMA GEMM through a workspace (the inverted-diagonal-
            // block scheme of vendor trsm), instead of n/64 waves each running an
            // m^2/2-long dependent chain
            Buffer W(dev, (size_t)m * m * es, s);
            check(kern::trsm_local((int)t, true, lower, trans, unit, m, m, A, lda, W.data(), m, s), "trsm_local");
            ApplyInverse(dev, t, m, n, W.data(), m, B, ldb, s);
            return;
        }
        check(kern::trsm_local((int)t, false, lower, trans, unit, m, n, A, lda, B, ldb, s), "trsm_local");
        return;
    }
    if (t == DType::F64)
        cpu_trsm(lower, trans, unit, m, n, static_cast<const double*>(A), lda, static_cast<double*>(B), ldb);
    else
        cpu_trsm(lower, trans, unit, m, n, static_cast<const float*>(A), lda, static_cast<float*>(B), ldb);
}

// Reads only the stored triangle (and no diagonal when unit).  In place: with
// op(A) lower, row i needs rows <= i of the old B, so rows go bottom to top;
// with op(A) upper, top to bottom.
template <typename S>
void cpu_trmm(bool lower, bool trans, bool unit, Int m, Int n, S alpha, const S* A, Int lda, S* B, Int ldb) {
    const bool op_lower = lower != trans;
    auto opA = [&](Int r, Int c) { return trans ? A[c + r * lda] : A[r + c * lda]; };
    for (Int j = 0; j < n; ++j) {
        S* x = B + j * ldb;
        for (Int s = 0; s < m; ++s) {
            const Int i = op_lower ? m - 1 - s : s;
            S acc = unit ? x[i] : opA(i, i) * x[i];
            if (op_lower)
                for (Int k = 0; k < i; ++k) acc += opA(i, k) * x[k];
            else
                for (Int k = i + 1; k < m; ++k) acc += opA(i, k) * x[k];
            x[i] = alpha * acc;
        }
    }
}

void Trmm(Device dev, DType t, bool lower, bool trans, bool unit, Int m, Int n, double alpha, const void* A, Int lda,
          void* B, Int ldb, hipStream_t s) {
    if (t != DType::F64 && t != DType::F32) throw LogicError("Trmm: only float and double are supported");
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) {
        // the kernel's output may not overlap B: into a workspace, then one copy back
        Buffer W(dev, (size_t)m * n * DTypeSize(t), s);
        check(kern::trmm_tri((int)t, lower, trans, unit, m, n, alpha, A, lda, B, ldb, W.data(), m, s), "trmm_tri");
        const Copy2D d{m, n, W.data(), 1, m, B, 1, ldb};
        Copy2DBatch(dev, t, &d, 1, false, 0.0, s);
        return;
    }
    if (t == DType::F64)
        cpu_trmm(lower, trans, unit, m, n, alpha, static_cast<const double*>(A), lda, static_cast<double*>(B), ldb);
    else
        cpu_trmm(lower, trans, unit, m, n, (float)alpha, static_cast<const float*>(A), lda, static_cast<float*>(B),
                 ldb);
}

// LowerVariant3Unblocked (LowerVariant3.hpp:24-50) on the stored triangle:
// S(i,j), i >= j, is A(i,j) when lower and A(j,i) when upper (A = U^T U)
template <typename S>
void cpu_cholesky(bool lower, Int n, S* A, Int lda, int* info, int col0) {
    auto a = [&](Int i, Int j) -> S& { return lower ? A[i + j * lda] : A[j + i * lda]; };
    for (Int j = 0; j < n; ++j) {
        const S d = a(j, j);
        if (!(d > S(0))) {
            if (*info == 0) *info = col0 + (int)j + 1;
            return;
        }
        const S sd = std::sqrt(d), inv = S(1) / sd;
        a(j, j) = sd;
        for (Int i = j + 1; i < n; ++i) a(i, j) *= inv;
        for (Int k = j + 1; k < n; ++k)
            for (Int i = k; i < n; ++i) a(i, k) -= a(i, j) * a(k, j);
    }
}

void Cholesky(Device dev, DType t, bool lower, Int n, void* A, Int lda, int* info, int col0, hipStream_t s) {
    if (t != DType::F64 && t != DType::F32) throw LogicError("Cholesky: only float and double are supported");
    if (n <= 0) return;
    if (dev == Device::GPU) {
        ELX_REQUIRE(n <= kern::kPotrfMax, "Cholesky: block of ", n, " rows exceeds ", kern::kPotrfMax);
        check(kern::potrf_block((int)t, lower, n, A, lda, info, col0, s), "potrf_block");
        return;
    }
    if (*info != 0) return;
    if (t == DType::F64) cpu_cholesky(lower, n, static_cast<double*>(A), lda, info, col0);
    else cpu_cholesky(lower, n, static_cast<float*>(A), lda, info, col0);
}

// lu::Panel (LU/Panel.hpp): per column the entry of largest magnitude at or
// below the diagonal (the first of equals; a NaN never beats a number), the row
// swap across the panel, the scaling and the rank-one update
template <typename S>
void cpu_lu_panel(Int m, Int w, S* A, Int lda, int* piv, int row_off, int* info, int col0) {
    for (Int j = 0; j < w; ++j) {
        S* aj = A + j * lda;
        Int p = -1;
        S best = S(-1);
        for (Int i = j; i < m; ++i) {
            const S v = std::fabs(aj[i]);
            if (v > best) { best = v; p = i; }
        }
        if (!(best > S(0))) {
            if (*info == 0) *info = col0 + (int)j + 1;
            return;
        }
        piv[j] = row_off + (int)p;
        if (p != j)
            for (Int k = 0; k < w; ++k) std::swap(A[j + k * lda], A[p + k * lda]);
        const S d = aj[j];
        for (Int i = j + 1; i < m; ++i) aj[i] = aj[i] / d;
        for (Int k = j + 1; k < w; ++k) {
            S* ak = A + k * lda;
            const S u = ak[j];
            for (Int i = j + 1; i < m; ++i) ak[i] -= aj[i] * u;
        }
    }
}

size_t LUWorkBytes(Device dev, Int m) { return dev == Device::GPU ? kern::getrf_work_bytes(m) : 0; }

void LU(Device dev, DType t, Int m, Int w, void* A, Int lda, int* piv, int row_off, void* work, int* info, int col0,
        hipStream_t s) {
    if (t != DType::F64 && t != DType::F32) throw LogicError("LU: only float and double are supported");
    if (m <= 0 || w <= 0) return;
    ELX_REQUIRE(w <= kern::kGetrfLeafCols && w <= m, "LU: a leaf of ", m, " x ", w);
    if (dev == Device::GPU) {
        check(kern::getrf_leaf((int)t, m, w, A, lda, piv, row_off, work, info, col0, s), "getrf_leaf");
        return;
    }
    if (*info != 0) return;
    if (t == DType::F64) cpu_lu_panel(m, w, static_cast<double*>(A), lda, piv, row_off, info, col0);
    else cpu_lu_panel(m, w, static_cast<float*>(A), lda, piv, row_off, info, col0);
}

template <typename S>
void cpu_laswp(Int m, Int n, S* A, Int lda, const int* piv, Int k0, Int k1, Int voff, bool inverse) {
    for (Int q = k0; q < k1; ++q) {
        const Int k = inverse ? k0 + k1 - 1 - q : q, p = (Int)piv[k] - voff;
        if (p == k || p < 0 || p >= m || k >= m) continue;
        for (Int c = 0; c < n; ++c) std::swap(A[k + c * lda], A[p + c * lda]);
    }
}

void Laswp(Device dev, DType t, Int m, Int n, void* A, Int lda, const int* piv, Int k0, Int k1, Int voff, bool inverse,
           const int* info, hipStream_t s) {
    if (t != DType::F64 && t != DType::F32) throw LogicError("Laswp: only float and double are supported");
    if (m <= 0 || n <= 0 || k1 <= k0) return;
    if (dev == Device::GPU) {
        check(kern::laswp((int)t, m, n, A, lda, piv, k0, k1, voff, inverse, info, s), "laswp");
        return;
    }
    if (info && *info != 0) return;
    // moved as integers: a swap through a float register may quieten a NaN on the host
    if (t == DType::F64) cpu_laswp(m, n, static_cast<uint64_t*>(A), lda, piv, k0, k1, voff, inverse);
    else cpu_laswp(m, n, static_cast<uint32_t*>(A), lda, piv, k0, k1, voff, inverse);
}

// qr::PanelHouseholder with reflector::Col, column by column; the norm as the
// scaled pair (max |a|, sum (a / max)^2), the dots with the already scaled u
// (|u_i| <= 1), sums in double
template <typename S>
void cpu_qr_panel(Int m, Int w, S* A, Int lda, S* tau, S* sig) {
    const Int k = std::min(m, w);
    for (Int j = 0; j < k; ++j) {
        S* aj = A + j * lda;
        double mx = 0.0;
        for (Int i = j + 1; i < m; ++i) {
            const double v = std::fabs((double)aj[i]);
            if (v > mx || v != v) mx = v;  // a NaN stays
        }
        const double alpha = (double)aj[j];
        double beta, t;
        if (mx == 0.0) {
            beta = -alpha;
            t = 2.0;
            for (Int i = j + 1; i < m; ++i) aj[i] = S(0);
        } else {
            double ssq = 0.0;
            for (Int i = j + 1; i < m; ++i) {
                const double r = (double)aj[i] / mx;
                ssq += r * r;
            }
            const double nrm = std::hypot(alpha, mx * std::sqrt(ssq));
            beta = alpha <= 0.0 ? nrm : -nrm;
            t = (double)(S)((beta - alpha) / beta);
            const double denom = alpha - beta;
            for (Int i = j + 1; i < m; ++i) aj[i] = (S)((double)aj[i] / denom);
        }
        const double d = beta >= 0.0 ? 1.0 : -1.0;
        for (Int c = j + 1; c < w; ++c) {
            S* ac = A + c * lda;
            double z = (double)ac[j];
            for (Int i = j + 1; i < m; ++i) z += (double)aj[i] * (double)ac[i];
            for (Int i = j + 1; i < m; ++i) ac[i] = (S)((double)ac[i] - t * (double)aj[i] * z);
            ac[j] = (S)(d * ((double)ac[j] - t * z));
        }
        aj[j] = (S)(beta * d);
        tau[j] = (S)t;
        sig[j] = (S)d;
    }
}

size_t QRWorkBytes(Device dev, Int m) { return dev == Device::GPU ? kern::geqrf_work_bytes(m) : 0; }

void QR(Device dev, DType t, Int m, Int w, void* A, Int lda, void* tau, void* sig, void* work, hipStream_t s) {
    if (t != DType::F64 && t != DType::F32) throw LogicError("QR: only float and double are supported");
    if (m <= 0 || w <= 0) return;
    ELX_REQUIRE(w <= kern::kGeqrfLeafCols, "QR: a leaf of ", m, " x ", w);
    if (dev == Device::GPU) {
        check(kern::geqrf_leaf((int)t, m, w, A, lda, tau, sig, work, s), "geqrf_leaf");
        return;
    }
    if (t == DType::F64)
        cpu_qr_panel(m, w, static_cast<double*>(A), lda, static_cast<double*>(tau), static_cast<double*>(sig));
    else cpu_qr_panel(m, w, static_cast<float*>(A), lda, static_cast<float*>(tau), static_cast<float*>(sig));
}

template <typename S>
void cpu_qr_explicit_u(Int m, Int nb, const S* A, Int lda, S* U, Int ldu) {
    for (Int c = 0; c < nb; ++c)
        for (Int i = 0; i < m; ++i) U[i + c * ldu] = i > c ? A[i + c * lda] : (i == c ? S(1) : S(0));
}

void QRExplicitU(Device dev, DType t, Int m, Int nb, const void* A, Int lda, void* U, Int ldu, hipStream_t s) {
    if (t != DType::F64 && t != DType::F32) throw LogicError("QR: only float and double are supported");
    if (m <= 0 || nb <= 0) return;
    if (dev == Device::GPU) {
        check(kern::qr_explicit_u((int)t, m, nb, A, lda, U, ldu, s), "qr_explicit_u");
        return;
    }
    if (t == DType::F64) cpu_qr_explicit_u(m, nb, static_cast<const double*>(A), lda, static_cast<double*>(U), ldu);
    else cpu_qr_explicit_u(m, nb, static_cast<const float*>(A), lda, static_cast<float*>(U), ldu);
}

template <typename S>
void cpu_qr_fix_t(Int nb, S* T, Int ldt, const S* tau) {
    for (Int c = 0; c < nb; ++c) {
        for (Int i = 0; i < c; ++i) T[i + c * ldt] = S(0);
        T[c + c * ldt] = S(1) / tau[c];
    }
}

void QRFixT(Device dev, DType t, Int nb, void* S, Int lds, const void* tau, hipStream_t s) {
    if (t != DType::F64 && t != DType::F32) throw LogicError("QR: only float and double are supported");
    if (nb <= 0) return;
    if (dev == Device::GPU) {
        check(kern::qr_fix_t((int)t, nb, S, lds, tau, s), "qr_fix_t");
        return;
    }
    if (t == DType::F64) cpu_qr_fix_t(nb, static_cast<double*>(S), lds, static_cast<const double*>(tau));
    else cpu_qr_fix_t(nb, static_cast<float*>(S), lds, static_cast<const float*>(tau));
}

template <typename S>
void cpu_row_scale(Int m, Int n, S* A, Int lda, const S* sig, Int i0, Int is) {
    for (Int c = 0; c < n; ++c)
        for (Int i = 0; i < m; ++i) A[i + c * lda] *= sig[i0 + i * is];
}

void RowScale(Device dev, DType t, Int m, Int n, void* A, Int lda, const void* sig, Int i0, Int is, hipStream_t s) {
    if (t != DType::F64 && t != DType::F32) throw LogicError("QR: only float and double are supported");
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) {
        check(kern::row_scale((int)t, m, n, A, lda, sig, i0, is, s), "row_scale");
        return;
    }
    if (t == DType::F64) cpu_row_scale(m, n, static_cast<double*>(A), lda, static_cast<const double*>(sig), i0, is);
    else cpu_row_scale(m, n, static_cast<float*>(A), lda, static_cast<const float*>(sig), i0, is);
}

// triang_inv::LVar3Unb (Inverse/Triangular/LVar3.hpp:17-43) on the stored
// triangle: S(i,j), i >= j, is A(i,j) when lower and A(j,i) when upper (UVar3Unb
// is the same loop on the transpose).  Divides without a singularity test.
template <typename S>
void cpu_trtri(bool lower, bool unit, Int n, S* A, Int lda) {
    auto a = [&](Int i, Int j) -> S& { return lower ? A[i + j * lda] : A[j + i * lda]; };
    for (Int j = 0; j < n; ++j) {
        const S lambda = unit ? S(1) : a(j, j);
        for (Int k = 0; k < j; ++k) a(j, k) /= -lambda;
        for (Int k = 0; k < j; ++k)
            for (Int i = j + 1; i < n; ++i) a(i, k) += a(i, j) * a(j, k);
        if (!unit) {
            for (Int i = j + 1; i < n; ++i) a(i, j) /= lambda;
            a(j, j) = S(1) / lambda;
        }
    }
}

void TriangularInverse(Device dev, DType t, bool lower, bool unit, Int n, void* A, Int lda, hipStream_t s) {
    if (t != DType::F64 && t != DType::F32) throw LogicError("TriangularInverse: only float and double are supported");
    if (n <= 0) return;
    if (dev == Device::GPU) {
        ELX_REQUIRE(n <= kern::kTrtriMax, "TriangularInverse: block of ", n, " rows exceeds ", kern::kTrtriMax);
        check(kern::trtri_block((int)t, lower, unit, n, A, lda, s), "trtri_block");
        return;
    }
    if (t == DType::F64) cpu_trtri(lower, unit, n, static_cast<double*>(A), lda);
    else cpu_trtri(lower, unit, n, static_cast<float*>(A), lda);
}

// trtrmm::LUnblocked (Trtrmm/Unblocked.hpp:16-64) on the stored triangle, S as
// in cpu_trtri (UUnblocked is the same loop on the transpose)
template <typename S>
void cpu_trtrmm(bool lower, Int n, S* A, Int lda) {
    auto a = [&](Int i, Int j) -> S& { return lower ? A[i + j * lda] : A[j + i * lda]; };
    for (Int j = 0; j < n; ++j) {
        for (Int k = 0; k < j; ++k) {
            const S gamma = a(j, k);
            for (Int i = k; i < j; ++i) a(i, k) += a(j, i) * gamma;
        }
        const S lambda = a(j, j);
        for (Int k = 0; k < j; ++k) a(j, k) *= lambda;
        a(j, j) = lambda * lambda;
    }
}

void Trtrmm(Device dev, DType t, bool lower, Int n, void* A, Int lda, hipStream_t s) {
    if (t != DType::F64 && t != DType::F32) throw LogicError("Trtrmm: only float and double are supported");
    if (n <= 0) return;
    if (dev == Device::GPU) {
        ELX_REQUIRE(n <= kern::kTrtriMax, "Trtrmm: block of ", n, " rows exceeds ", kern::kTrtriMax);
        check(kern::lauum_block((int)t, lower, n, A, lda, s), "lauum_block");
        return;
    }
    if (t == DType::F64) cpu_trtrmm(lower, n, static_cast<double*>(A), lda);
    else cpu_trtrmm(lower, n, static_cast<float*>(A), lda);
}

void TriInverseBatched(DType t, bool lower, bool trans, bool unit, Int nb, Int m, const void* A, Int lda, void* W,
                       hipStream_t s) {
    check(kern::tri_inverse_batched((int)t, lower, trans, unit, nb, m, A, lda, W, s), "tri_inverse_batched");
}

void ApplyInverse(Device dev, DType t, Int m, Int n, const void* W, Int ldw, void* B, Int ldb, hipStream_t s) {
    if (m <= 0 || n <= 0) return;
    Buffer T(dev, (size_t)m * n * DTypeSize(t), s);
    Gemm(dev, t, false, false, m, n, m, 1.0, W, ldw, B, ldb, 0.0, T.data(), m, s);
    const Copy2D d{m, n, T.data(), 1, m, B, 1, ldb};
    Copy2DBatch(dev, t, &d, 1, false, 0.0, s);
}

void FillHash(Device dev, DType t, Int m, Int n, void* A, Int lda, Int i0, Int is, Int j0, Int js,
              uint64_t seed, double center, double radius, hipStream_t s) {
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) {
        check(kern::fill_hash((int)t, m, n, A, lda, i0, is, j0, js, seed, center, radius, s), "fill_hash");
        return;
    }
    HOST_DTYPE_SWITCH(t, S, {
        S* a = static_cast<S*>(A);
        for (Int j = 0; j < n; ++j)
            for (Int i = 0; i < m; ++i) {
                const double u = kern::hash_unit(seed, i0 + i * is, j0 + j * js);
                H<S>::st(a + i + j * lda, (typename H<S>::C)(center + radius * (2.0 * u - 1.0)));
            }
    });
}

namespace {
void RequireReal(DType t, const char* who) {
    if (t != DType::F64 && t != DType::F32) throw LogicError(Cat(who, ": only float and double are supported"));
}
template <typename S>
void cpu_vec_scale(Int len, double beta, S* y, Int incy) {
    using Cm = typename H<S>::C;
    if (beta == 1.0) return;
    for (Int i = 0; i < len; ++i) H<S>::st(y + i * incy, beta == 0.0 ? Cm(0) : (Cm)beta * H<S>::ld(y + i * incy));
}
template <typename S>
void cpu_finish(S* y, double alpha, typename H<S>::C acc, double beta) {
    using Cm = typename H<S>::C;
    H<S>::st(y, beta == 0.0 ? (Cm)alpha * acc : (Cm)alpha * acc + (Cm)beta * H<S>::ld(y));
}
template <typename S>
void cpu_gemv(bool trans, Int m, Int n, double alpha, const S* A, Int lda, const S* x, Int incx, double beta, S* y,
              Int incy) {
    using Cm = typename H<S>::C;
    if (trans) {
        for (Int j = 0; j < n; ++j) {
            Cm acc = Cm(0);
            for (Int i = 0; i < m; ++i) acc += H<S>::ld(A + i + j * lda) * H<S>::ld(x + i * incx);
            cpu_finish(y + j * incy, alpha, acc, beta);
        }
        return;
    }
    std::vector<Cm> acc(static_cast<size_t>(m), Cm(0));
    for (Int j = 0; j < n; ++j) {
        const Cm xv = H<S>::ld(x + j * incx);
        for (Int i = 0; i < m; ++i) acc[i] += H<S>::ld(A + i + j * lda) * xv;
    }
    for (Int i = 0; i < m; ++i) cpu_finish(y + i * incy, alpha, acc[i], beta);
}
struct HostTri {
    bool lower;
    Int i0, is, j0, js;
    bool in(Int i, Int j) const { return lower ? i0 + i * is >= j0 + j * js : i0 + i * is <= j0 + j * js; }
    bool strict(Int i, Int j) const { return lower ? i0 + i * is > j0 + j * js : i0 + i * is < j0 + j * js; }
};
template <typename S>
void cpu_symv(const HostTri& tri, Int m, Int n, double alpha, const S* A, Int lda, const S* xr, Int incxr, const S* xc,
              Int incxc, double beta, S* zr, Int inczr, S* zc, Int inczc) {
    using Cm = typename H<S>::C;
    std::vector<Cm> ar(static_cast<size_t>(m), Cm(0)), ac(static_cast<size_t>(n), Cm(0));
    for (Int j = 0; j < n; ++j) {
        const Cm xv = H<S>::ld(xc + j * incxc);
        for (Int i = 0; i < m; ++i) {
            if (!tri.in(i, j)) continue;
            const Cm a = H<S>::ld(A + i + j * lda);
            ar[i] += a * xv;
            if (tri.strict(i, j)) ac[j] += a * H<S>::ld(xr + i * incxr);
        }
    }
    if (zc) {
        for (Int i = 0; i < m; ++i) cpu_finish(zr + i * inczr, alpha, ar[i], beta);
        for (Int j = 0; j < n; ++j) cpu_finish(zc + j * inczc, alpha, ac[j], beta);
    } else {
        for (Int i = 0; i < m; ++i) cpu_finish(zr + i * inczr, alpha, ar[i] + ac[i], beta);
    }
}
// terms 0: Ger (no triangle), 1: Syr, 2: Syr2
template <typename S>
void cpu_rank_update(int terms, const HostTri& tri, Int m, Int n, double alpha, const S* xr, Int incxr, const S* yc,
                     Int incyc, const S* yr, Int incyr, const S* xc, Int incxc, S* A, Int lda) {
    using Cm = typename H<S>::C;
    for (Int j = 0; j < n; ++j) {
        const Cm sv = H<S>::ld(yc + j * incyc), tv = terms == 2 ? H<S>::ld(xc + j * incxc) : Cm(0);
        for (Int i = 0; i < m; ++i) {
            if (terms != 0 && !tri.in(i, j)) continue;
            Cm z = H<S>::ld(A + i + j * lda) + ((Cm)alpha * H<S>::ld(xr + i * incxr)) * sv;
            if (terms == 2) z += ((Cm)alpha * H<S>::ld(yr + i * incyr)) * tv;
            H<S>::st(A + i + j * lda, z);
        }
    }
}
void RankUpdate(const char* who, Device dev, DType t, int terms, bool lower, Int m, Int n, double alpha, const void* xr,
                Int incxr, const void* yc, Int incyc, const void* yr, Int incyr, const void* xc, Int incxc, void* A,
                Int lda, Int i0, Int is, Int j0, Int js, hipStream_t s) {
    RequireReal(t, who);
    if (m <= 0 || n <= 0 || alpha == 0.0) return;
    if (dev == Device::GPU) {
        check(kern::rank_update((int)t, terms, lower, m, n, alpha, xr, incxr, yc, incyc, yr, incyr, xc, incxc, A, lda,
                                i0, is, j0, js, s),
              who);
        return;
    }
    const HostTri tri{lower, i0, is, j0, js};
    HOST_DTYPE_SWITCH(t, S,
                      cpu_rank_update<S>(terms, tri, m, n, alpha, static_cast<const S*>(xr), incxr,
                                         static_cast<const S*>(yc), incyc, static_cast<const S*>(yr), incyr,
                                         static_cast<const S*>(xc), incxc, static_cast<S*>(A), lda));
}
}  // namespace

void Gemv(Device dev, DType t, bool trans, Int m, Int n, double alpha, const void* A, Int lda, const void* x, Int incx,
          double beta, void* y, Int incy, hipStream_t s) {
    const Int ylen = trans ? n : m, xlen = trans ? m : n;
    if (ylen <= 0) return;
    if (dev == Device::GPU) {
        check(kern::gemv((int)t, trans, m, n, alpha, A, lda, x, incx, beta, y, incy, s), "gemv");
        return;
    }
    HOST_DTYPE_SWITCH(t, S, {
        if (xlen <= 0 || alpha == 0.0) cpu_vec_scale<S>(ylen, beta, static_cast<S*>(y), incy);
        else cpu_gemv<S>(trans, m, n, alpha, static_cast<const S*>(A), lda, static_cast<const S*>(x), incx, beta,
                         static_cast<S*>(y), incy);
    });
}

void Ger(Device dev, DType t, Int m, Int n, double alpha, const void* x, Int incx, const void* y, Int incy, void* A,
         Int lda, hipStream_t s) {
    RankUpdate("Ger", dev, t, 0, true, m, n, alpha, x, incx, y, incy, nullptr, 1, nullptr, 1, A, lda, 0, 1, 0, 1, s);
}

void SymvAccumulate(Device dev, DType t, bool lower, Int m, Int n, double alpha, const void* A, Int lda,
                    const void* xr, Int incxr, const void* xc, Int incxc, double beta, void* zr, Int inczr, void* zc,
                    Int inczc, Int i0, Int is, Int j0, Int js, hipStream_t s) {
    RequireReal(t, "Symv");
    ELX_REQUIRE(zc != nullptr || m == n, "Symv: one output vector needs a square block, got ", m, " x ", n);
    if (dev == Device::GPU) {
        check(kern::symv((int)t, lower, m, n, alpha, A, lda, xr, incxr, xc, incxc, beta, zr, inczr, zc, inczc, i0, is,
                         j0, js, s),
              "symv");
        return;
    }
    HOST_DTYPE_SWITCH(t, S, {
        if (m <= 0 || n <= 0 || alpha == 0.0) {
            cpu_vec_scale<S>(m, beta, static_cast<S*>(zr), inczr);
            if (zc) cpu_vec_scale<S>(n, beta, static_cast<S*>(zc), inczc);
        } else {
            cpu_symv<S>(HostTri{lower, i0, is, j0, js}, m, n, alpha, static_cast<const S*>(A), lda,
                        static_cast<const S*>(xr), incxr, static_cast<const S*>(xc), incxc, beta, static_cast<S*>(zr),
                        inczr, static_cast<S*>(zc), inczc);
        }
    });
}

void Syr(Device dev, DType t, bool lower, Int m, Int n, double alpha, const void* xr, Int incxr, const void* xc,
         Int incxc, void* A, Int lda, Int i0, Int is, Int j0, Int js, hipStream_t s) {
    RankUpdate("Syr", dev, t, 1, lower, m, n, alpha, xr, incxr, xc, incxc, nullptr, 1, nullptr, 1, A, lda, i0, is, j0,
               js, s);
}

void Syr2(Device dev, DType t, bool lower, Int m, Int n, double alpha, const void* xr, Int incxr, const void* xc,
          Int incxc, const void* yr, Int incyr, const void* yc, Int incyc, void* A, Int lda, Int i0, Int is, Int j0,
          Int js, hipStream_t s) {
    RankUpdate("Syr2", dev, t, 2, lower, m, n, alpha, xr, incxr, yc, incyc, yr, incyr, xc, incxc, A, lda, i0, is, j0, js,
               s);
}

double LoadScalar(DType t, const void* p) {
    double v = 0;
    HOST_DTYPE_SWITCH(t, S, v = (double)H<S>::ld(static_cast<const S*>(p)));
    return v;
}
void StoreScalar(DType t, void* p, double v) {
    HOST_DTYPE_SWITCH(t, S, H<S>::st(static_cast<S*>(p), (typename H<S>::C)v));
}

}  // namespace exec
}  // namespace elx
