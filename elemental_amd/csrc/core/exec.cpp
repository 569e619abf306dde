// The Device::GPU / Device::CPU dispatch of every local primitive.  The host
// loops themselves live in host_elem.hpp, host_blas.hpp and host_leaves.hpp.
#include <cstdlib>
#include "exec.hpp"
#include "strassen.hpp"
#include "host_blas.hpp"
#include "host_leaves.hpp"
#include <cmath>
#include <type_traits>
#include <vector>

namespace elx {
namespace exec {

namespace {

[[noreturn]] void NotAMatrixType(DType t) { throw LogicError(Cat("dtype ", DTypeName(t), " is not a matrix type")); }
// exec's form of the dtype switch: an unknown code throws
#define EXEC_SWITCH(t, T, ...) ELX_DTYPE_SWITCH(t, T, NotAMatrixType(t), __VA_ARGS__)
#define EXEC_REAL_SWITCH(t, T, ...) ELX_REAL_SWITCH(t, T, NotAMatrixType(t), __VA_ARGS__)

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
    for (int q = 0; q < nd; ++q) EXEC_SWITCH(t, T, cpu_copy<T>(d[q], axpy, alpha));
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
        EXEC_SWITCH(t, T, cpu_copy<T>(d, true, alpha));
    }
}

void Convert2D(Device dev, DType src_t, DType dst_t, const Copy2D& d, hipStream_t s) {
    if (d.m <= 0 || d.n <= 0) return;
    if (src_t == dst_t) { Copy2DBatch(dev, src_t, &d, 1, false, 0.0, s); return; }
    if (dev == Device::GPU) {
        check(kern::convert2d(static_cast<int>(src_t), static_cast<int>(dst_t), d, s), "convert2d");
        return;
    }
    EXEC_SWITCH(src_t, TS, EXEC_SWITCH(dst_t, TD, cpu_convert<TS, TD>(d)));
}

namespace {
thread_local int t_gemm_levels = 0;
}
int GemmLastLevels() { return t_gemm_levels; }

void Gemm(Device dev, DType t, bool ta, bool tb, Int m, Int n, Int k, double alpha, const void* A, Int lda,
          const void* B, Int ldb, double beta, void* C, Int ldc, hipStream_t s) {
    t_gemm_levels = 0;
    if (m <= 0 || n <= 0) return;
    // the knobs are read per call (two getenv), and only for the types that can take the path
    if (k >= 2 && (t == DType::F64 || t == DType::F32)) {
        const strassen::Knobs kn = strassen::ReadKnobs();
        t_gemm_levels = strassen::Gemm(kn.levels, kn, dev, t, ta, tb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, s);
        if (t_gemm_levels > 0) return;
    }
    GemmPlain(dev, t, ta, tb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, s);
}

void QuadSum(Device dev, DType t, const kern::QuadSum* q, int nq, hipStream_t s) {
    RequireReal(t, "QuadSum");
    if (dev == Device::GPU) { check(kern::quad_sum((int)t, q, nq, s), "quad_sum"); return; }
    for (int d = 0; d < nq; ++d)
        EXEC_REAL_SWITCH(t, T, {
            const kern::QuadSum& a = q[d];
            const T* x = static_cast<const T*>(a.x);
            const T* y = static_cast<const T*>(a.y);
            T* o = static_cast<T*>(a.d);
            for (Int j = 0; j < a.n; ++j)
                for (Int i = 0; i < a.m; ++i) o[i + j * a.ldd] = x[i + j * a.ldx] + (T)a.sy * y[i + j * a.ldy];
        });
}

void QuadScatter(Device dev, DType t, const kern::QuadScatter& q, hipStream_t s) {
    RequireReal(t, "QuadScatter");
    if (dev == Device::GPU) { check(kern::quad_scatter((int)t, q, s), "quad_scatter"); return; }
    EXEC_REAL_SWITCH(t, T, {
        const T* M = static_cast<const T*>(q.M);
        for (int w = 0; w < q.nt; ++w) {
            T* c = static_cast<T*>(q.c[w]);
            for (Int j = 0; j < q.n; ++j)
                for (Int i = 0; i < q.m; ++i) {
                    T v = (T)q.coef[w] * M[i + j * q.ldm];
                    if (q.beta[w] != 0.0) v = v + (T)q.beta[w] * c[i + j * q.ldc[w]];
                    c[i + j * q.ldc[w]] = v;
                }
        }
    });
}

void GemmPlain(Device dev, DType t, bool ta, bool tb, Int m, Int n, Int k, double alpha, const void* A, Int lda,
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
            NotAMatrixType(t);
        }
        check(e, "gemm_mfma");
        return;
    }
    EXEC_SWITCH(t, T,
        cpu_gemm<T>(ta, tb, m, n, k, alpha, static_cast<const Stor<T>*>(A), lda, static_cast<const Stor<T>*>(B), ldb,
                    beta, static_cast<Stor<T>*>(C), ldc));
}

void Fill(Device dev, DType t, Int m, Int n, double v, void* A, Int lda, hipStream_t s) {
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) { check(kern::fill2d((int)t, m, n, v, A, lda, s), "fill2d"); return; }
    EXEC_SWITCH(t, T, {
        auto* a = static_cast<Stor<T>*>(A);
        for (Int j = 0; j < n; ++j)
            for (Int i = 0; i < m; ++i) H<T>::st(a + i + j * lda, (typename H<T>::C)v);
    });
}

void Scale(Device dev, DType t, Int m, Int n, double alpha, void* A, Int lda, hipStream_t s) {
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) { check(kern::scale2d((int)t, m, n, alpha, A, lda, s), "scale2d"); return; }
    EXEC_SWITCH(t, T, {
        auto* a = static_cast<Stor<T>*>(A);
        using Cm = typename H<T>::C;
        for (Int j = 0; j < n; ++j)
            for (Int i = 0; i < m; ++i) H<T>::st(a + i + j * lda, (Cm)alpha * H<T>::ld(a + i + j * lda));
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
    EXEC_SWITCH(t, T, {
        const auto* a = static_cast<const Stor<T>*>(A);
        for (Int j = 0; j < n; ++j)
            for (Int i = 0; i < m; ++i) {
                const double x = (double)H<T>::ld(a + i + j * lda);
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
    EXEC_SWITCH(t, T, {
        const auto* a = static_cast<const Stor<T>*>(A);
        const auto* b = static_cast<const Stor<T>*>(B);
        auto* c = static_cast<Stor<T>*>(C);
        for (Int j = 0; j < n; ++j)
            for (Int i = 0; i < m; ++i)
                H<T>::st(c + i + j * ldc, H<T>::ld(a + i + j * lda) * H<T>::ld(b + i + j * ldb));
    });
}

void Map(Device dev, DType t, int fn, Int m, Int n, const void* A, Int lda, void* B, Int ldb, hipStream_t s) {
    if (fn < ELX_MAP_IDENTITY || fn > ELX_MAP_TANH) throw LogicError(Cat("unknown entrywise functor ", fn));
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) { check(kern::entrywise_map((int)t, fn, m, n, A, lda, B, ldb, s), "entrywise_map"); return; }
    EXEC_SWITCH(t, T, {
        const auto* a = static_cast<const Stor<T>*>(A);
        auto* b = static_cast<Stor<T>*>(B);
        for (Int j = 0; j < n; ++j)
            for (Int i = 0; i < m; ++i) H<T>::st(b + i + j * ldb, cpu_map(fn, H<T>::ld(a + i + j * lda)));
    });
}

void Combine(Device dev, DType t, int fn, Int m, Int n, const void* A, Int lda, void* B, Int ldb, hipStream_t s) {
    if (fn < ELX_COMBINE_ADD || fn > ELX_COMBINE_RELU_GRAD) throw LogicError(Cat("unknown combine functor ", fn));
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) { check(kern::combine((int)t, fn, m, n, A, lda, B, ldb, s), "combine"); return; }
    EXEC_SWITCH(t, T, {
        const auto* a = static_cast<const Stor<T>*>(A);
        auto* b = static_cast<Stor<T>*>(B);
        for (Int j = 0; j < n; ++j)
            for (Int i = 0; i < m; ++i)
                H<T>::st(b + i + j * ldb, cpu_combine(fn, H<T>::ld(a + i + j * lda), H<T>::ld(b + i + j * ldb)));
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
    EXEC_SWITCH(t, T, {
        using Cm = typename H<T>::C;
        const auto* x = static_cast<const Stor<T>*>(X);
        auto* y = static_cast<Stor<T>*>(Y);
        for (Int j = 0; j < n; ++j)
            for (Int i = 0; i < m; ++i) {
                const Int gi = i0 + i * is, gj = j0 + j * js - offset;
                if (lower ? gi < gj : gi > gj) continue;
                Cm v = (x && beta == 0.0) ? Cm(0) : (Cm)beta * H<T>::ld(y + i + j * ldy);
                if (x) v = v + (Cm)alpha * H<T>::ld(x + i + j * ldx);
                H<T>::st(y + i + j * ldy, v);
            }
    });
}

void Trsm(Device dev, DType t, bool lower, bool trans, bool unit, Int m, Int n, const void* A, Int lda, void* B,
          Int ldb, hipStream_t s) {
    RequireReal(t, "Trsm");
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) {
        const size_t es = DTypeSize(t);
        if (kern::trsm_plan(es, m, n).invert) {
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
    EXEC_REAL_SWITCH(t, T, cpu_trsm(lower, trans, unit, m, n, static_cast<const T*>(A), lda, static_cast<T*>(B), ldb));
}

void Trmm(Device dev, DType t, bool lower, bool trans, bool unit, Int m, Int n, double alpha, const void* A, Int lda,
          void* B, Int ldb, hipStream_t s) {
    RequireReal(t, "Trmm");
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) {
        // the kernel's output may not overlap B: into a workspace, then one copy back
        Buffer W(dev, (size_t)m * n * DTypeSize(t), s);
        check(kern::trmm_tri((int)t, lower, trans, unit, m, n, alpha, A, lda, B, ldb, W.data(), m, s), "trmm_tri");
        const Copy2D d{m, n, W.data(), 1, m, B, 1, ldb};
        Copy2DBatch(dev, t, &d, 1, false, 0.0, s);
        return;
    }
    EXEC_REAL_SWITCH(t, T, cpu_trmm(lower, trans, unit, m, n, (T)alpha, static_cast<const T*>(A), lda,
                                    static_cast<T*>(B), ldb));
}

void Cholesky(Device dev, DType t, bool lower, Int n, void* A, Int lda, int* info, int col0, hipStream_t s) {
    RequireReal(t, "Cholesky");
    if (n <= 0) return;
    if (dev == Device::GPU) {
        ELX_REQUIRE(n <= kern::kPotrfMax, "Cholesky: block of ", n, " rows exceeds ", kern::kPotrfMax);
        check(kern::potrf_block((int)t, lower, n, A, lda, info, col0, s), "potrf_block");
        return;
    }
    if (*info != 0) return;
    EXEC_REAL_SWITCH(t, T, cpu_cholesky(lower, n, static_cast<T*>(A), lda, info, col0));
}

size_t LUWorkBytes(Device dev, Int m) { return dev == Device::GPU ? kern::getrf_work_bytes(m) : 0; }

void LU(Device dev, DType t, Int m, Int w, void* A, Int lda, int* piv, int row_off, void* work, int* info, int col0,
        hipStream_t s) {
    RequireReal(t, "LU");
    if (m <= 0 || w <= 0) return;
    ELX_REQUIRE(w <= kern::kGetrfLeafCols && w <= m, "LU: a leaf of ", m, " x ", w);
    if (dev == Device::GPU) {
        check(kern::getrf_leaf((int)t, m, w, A, lda, piv, row_off, work, info, col0, s), "getrf_leaf");
        return;
    }
    if (*info != 0) return;
    EXEC_REAL_SWITCH(t, T, cpu_lu_panel(m, w, static_cast<T*>(A), lda, piv, row_off, info, col0));
}

void Laswp(Device dev, DType t, Int m, Int n, void* A, Int lda, const int* piv, Int k0, Int k1, Int voff, bool inverse,
           const int* info, hipStream_t s) {
    RequireReal(t, "Laswp");
    if (m <= 0 || n <= 0 || k1 <= k0) return;
    if (dev == Device::GPU) {
        check(kern::laswp((int)t, m, n, A, lda, piv, k0, k1, voff, inverse, info, s), "laswp");
        return;
    }
    if (info && *info != 0) return;
    // moved as integers: a swap through a float register may quieten a NaN on the host
    EXEC_REAL_SWITCH(t, T, {
        using U = typename std::conditional<sizeof(T) == 8, uint64_t, uint32_t>::type;
        cpu_laswp(m, n, static_cast<U*>(A), lda, piv, k0, k1, voff, inverse);
    });
}

size_t QRWorkBytes(Device dev, Int m) { return dev == Device::GPU ? kern::geqrf_work_bytes(m) : 0; }

void QR(Device dev, DType t, Int m, Int w, void* A, Int lda, void* tau, void* sig, void* work, hipStream_t s) {
    RequireReal(t, "QR");
    if (m <= 0 || w <= 0) return;
    ELX_REQUIRE(w <= kern::kGeqrfLeafCols, "QR: a leaf of ", m, " x ", w);
    if (dev == Device::GPU) {
        check(kern::geqrf_leaf((int)t, m, w, A, lda, tau, sig, work, s), "geqrf_leaf");
        return;
    }
    EXEC_REAL_SWITCH(t, T, cpu_qr_panel(m, w, static_cast<T*>(A), lda, static_cast<T*>(tau), static_cast<T*>(sig)));
}

void QRExplicitU(Device dev, DType t, Int m, Int nb, const void* A, Int lda, void* U, Int ldu, hipStream_t s,
                 bool upper, Int off) {
    RequireReal(t, "QR");
    if (m <= 0 || nb <= 0) return;
    if (dev == Device::GPU) {
        check(kern::qr_explicit_u((int)t, m, nb, A, lda, U, ldu, s, upper, off), "qr_explicit_u");
        return;
    }
    EXEC_REAL_SWITCH(t, T,
                     cpu_qr_explicit_u(m, nb, static_cast<const T*>(A), lda, static_cast<T*>(U), ldu, upper, off));
}

size_t SytrdWorkBytes(Int n) { return kern::sytrd_work_bytes(n); }

void SytrdPanel(DType t, bool lower, Int n, Int c0, Int w, void* A, Int lda, void* tau, void* V, void* W, Int ldv,
                void* work, hipStream_t s) {
    RequireReal(t, "HermitianTridiag");
    if (n <= 1 || w <= 0) return;
    check(kern::sytrd_panel((int)t, lower, n, c0, w, A, lda, tau, V, W, ldv, work, s), "sytrd_panel");
}

void HostHermitianTridiag(DType t, bool lower, Int n, void* A, Int lda, void* tau) {
    RequireReal(t, "HermitianTridiag");
    if (n <= 1) return;
    EXEC_REAL_SWITCH(t, T, cpu_sytrd(lower, n, static_cast<T*>(A), lda, static_cast<T*>(tau)));
}

void QRFixT(Device dev, DType t, Int nb, void* S, Int lds, const void* tau, hipStream_t s) {
    RequireReal(t, "QR");
    if (nb <= 0) return;
    if (dev == Device::GPU) {
        check(kern::qr_fix_t((int)t, nb, S, lds, tau, s), "qr_fix_t");
        return;
    }
    EXEC_REAL_SWITCH(t, T, cpu_qr_fix_t(nb, static_cast<T*>(S), lds, static_cast<const T*>(tau)));
}

void RowScale(Device dev, DType t, Int m, Int n, void* A, Int lda, const void* sig, Int i0, Int is, hipStream_t s) {
    RequireReal(t, "QR");
    if (m <= 0 || n <= 0) return;
    if (dev == Device::GPU) {
        check(kern::row_scale((int)t, m, n, A, lda, sig, i0, is, s), "row_scale");
        return;
    }
    EXEC_REAL_SWITCH(t, T, cpu_row_scale(m, n, static_cast<T*>(A), lda, static_cast<const T*>(sig), i0, is));
}

void TriangularInverse(Device dev, DType t, bool lower, bool unit, Int n, void* A, Int lda, hipStream_t s) {
    RequireReal(t, "TriangularInverse");
    if (n <= 0) return;
    if (dev == Device::GPU) {
        ELX_REQUIRE(n <= kern::kTrtriMax, "TriangularInverse: block of ", n, " rows exceeds ", kern::kTrtriMax);
        check(kern::trtri_block((int)t, lower, unit, n, A, lda, s), "trtri_block");
        return;
    }
    EXEC_REAL_SWITCH(t, T, cpu_trtri(lower, unit, n, static_cast<T*>(A), lda));
}

void Trtrmm(Device dev, DType t, bool lower, Int n, void* A, Int lda, hipStream_t s) {
    RequireReal(t, "Trtrmm");
    if (n <= 0) return;
    if (dev == Device::GPU) {
        ELX_REQUIRE(n <= kern::kTrtriMax, "Trtrmm: block of ", n, " rows exceeds ", kern::kTrtriMax);
        check(kern::lauum_block((int)t, lower, n, A, lda, s), "lauum_block");
        return;
    }
    EXEC_REAL_SWITCH(t, T, cpu_trtrmm(lower, n, static_cast<T*>(A), lda));
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
    EXEC_SWITCH(t, T, {
        auto* a = static_cast<Stor<T>*>(A);
        for (Int j = 0; j < n; ++j)
            for (Int i = 0; i < m; ++i) {
                const double u = kern::hash_unit(seed, i0 + i * is, j0 + j * js);
                H<T>::st(a + i + j * lda, (typename H<T>::C)(center + radius * (2.0 * u - 1.0)));
            }
    });
}

namespace {
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
    EXEC_REAL_SWITCH(t, T,
                     cpu_rank_update<T>(terms, tri, m, n, alpha, static_cast<const T*>(xr), incxr,
                                        static_cast<const T*>(yc), incyc, static_cast<const T*>(yr), incyr,
                                        static_cast<const T*>(xc), incxc, static_cast<T*>(A), lda));
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
    EXEC_SWITCH(t, T, {
        using S = Stor<T>;
        if (xlen <= 0 || alpha == 0.0) cpu_vec_scale<T>(ylen, beta, static_cast<S*>(y), incy);
        else cpu_gemv<T>(trans, m, n, alpha, static_cast<const S*>(A), lda, static_cast<const S*>(x), incx, beta,
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
    EXEC_REAL_SWITCH(t, T, {
        if (m <= 0 || n <= 0 || alpha == 0.0) {
            cpu_vec_scale<T>(m, beta, static_cast<T*>(zr), inczr);
            if (zc) cpu_vec_scale<T>(n, beta, static_cast<T*>(zc), inczc);
        } else {
            cpu_symv<T>(HostTri{lower, i0, is, j0, js}, m, n, alpha, static_cast<const T*>(A), lda,
                        static_cast<const T*>(xr), incxr, static_cast<const T*>(xc), incxc, beta, static_cast<T*>(zr),
                        inczr, static_cast<T*>(zc), inczc);
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
    EXEC_SWITCH(t, T, return (double)H<T>::ld(static_cast<const Stor<T>*>(p)));
}
void StoreScalar(DType t, void* p, double v) {
    EXEC_SWITCH(t, T, H<T>::st(static_cast<Stor<T>*>(p), (typename H<T>::C)v));
}

}  // namespace exec
}  // namespace elx
