// Device::CPU, levels 2 and 3: the reference loops behind exec::Gemm, Trsm,
// Trmm, Gemv, SymvAccumulate and the rank updates.  Sums run in the compute
// type of T, every result is rounded once into the storage type.
#pragma once
#include "host_elem.hpp"
#include <algorithm>
#include <vector>

namespace elx {
namespace exec {

template <typename T>
void cpu_gemm(bool ta, bool tb, Int m, Int n, Int k, double alpha, const Stor<T>* A, Int lda,
              const Stor<T>* B, Int ldb, double beta, Stor<T>* C, Int ldc) {
    using Cm = typename H<T>::C;
    std::vector<Cm> acc(static_cast<size_t>(m));
    for (Int j = 0; j < n; ++j) {
        std::fill(acc.begin(), acc.end(), Cm(0));
        for (Int l = 0; l < k; ++l) {
            const Cm b = H<T>::ld(tb ? B + j + l * ldb : B + l + j * ldb);
            if (b == Cm(0)) continue;
            if (!ta) {
                const auto* acol = A + l * lda;
                for (Int i = 0; i < m; ++i) acc[i] += H<T>::ld(acol + i) * b;
            } else {
                for (Int i = 0; i < m; ++i) acc[i] += H<T>::ld(A + l + i * lda) * b;
            }
        }
        for (Int i = 0; i < m; ++i) {
            auto* c = C + i + j * ldc;
            const Cm v = (Cm)alpha * acc[i];
            H<T>::st(c, beta == 0.0 ? v : v + (Cm)beta * H<T>::ld(c));
        }
    }
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

template <typename T>
void cpu_vec_scale(Int len, double beta, Stor<T>* y, Int incy) {
    using Cm = typename H<T>::C;
    if (beta == 1.0) return;
    for (Int i = 0; i < len; ++i) H<T>::st(y + i * incy, beta == 0.0 ? Cm(0) : (Cm)beta * H<T>::ld(y + i * incy));
}
template <typename T>
void cpu_finish(Stor<T>* y, double alpha, typename H<T>::C acc, double beta) {
    using Cm = typename H<T>::C;
    H<T>::st(y, beta == 0.0 ? (Cm)alpha * acc : (Cm)alpha * acc + (Cm)beta * H<T>::ld(y));
}
template <typename T>
void cpu_gemv(bool trans, Int m, Int n, double alpha, const Stor<T>* A, Int lda, const Stor<T>* x,
              Int incx, double beta, Stor<T>* y, Int incy) {
    using Cm = typename H<T>::C;
    if (trans) {
        for (Int j = 0; j < n; ++j) {
            Cm acc = Cm(0);
            for (Int i = 0; i < m; ++i) acc += H<T>::ld(A + i + j * lda) * H<T>::ld(x + i * incx);
            cpu_finish<T>(y + j * incy, alpha, acc, beta);
        }
        return;
    }
    std::vector<Cm> acc(static_cast<size_t>(m), Cm(0));
    for (Int j = 0; j < n; ++j) {
        const Cm xv = H<T>::ld(x + j * incx);
        for (Int i = 0; i < m; ++i) acc[i] += H<T>::ld(A + i + j * lda) * xv;
    }
    for (Int i = 0; i < m; ++i) cpu_finish<T>(y + i * incy, alpha, acc[i], beta);
}

struct HostTri {
    bool lower;
    Int i0, is, j0, js;
    bool in(Int i, Int j) const { return lower ? i0 + i * is >= j0 + j * js : i0 + i * is <= j0 + j * js; }
    bool strict(Int i, Int j) const { return lower ? i0 + i * is > j0 + j * js : i0 + i * is < j0 + j * js; }
};
template <typename T>
void cpu_symv(const HostTri& tri, Int m, Int n, double alpha, const Stor<T>* A, Int lda,
              const Stor<T>* xr, Int incxr, const Stor<T>* xc, Int incxc, double beta,
              Stor<T>* zr, Int inczr, Stor<T>* zc, Int inczc) {
    using Cm = typename H<T>::C;
    std::vector<Cm> ar(static_cast<size_t>(m), Cm(0)), ac(static_cast<size_t>(n), Cm(0));
    for (Int j = 0; j < n; ++j) {
        const Cm xv = H<T>::ld(xc + j * incxc);
        for (Int i = 0; i < m; ++i) {
            if (!tri.in(i, j)) continue;
            const Cm a = H<T>::ld(A + i + j * lda);
            ar[i] += a * xv;
            if (tri.strict(i, j)) ac[j] += a * H<T>::ld(xr + i * incxr);
        }
    }
    if (zc) {
        for (Int i = 0; i < m; ++i) cpu_finish<T>(zr + i * inczr, alpha, ar[i], beta);
        for (Int j = 0; j < n; ++j) cpu_finish<T>(zc + j * inczc, alpha, ac[j], beta);
    } else {
        for (Int i = 0; i < m; ++i) cpu_finish<T>(zr + i * inczr, alpha, ar[i] + ac[i], beta);
    }
}
// terms 0: Ger (no triangle), 1: Syr, 2: Syr2
template <typename T>
void cpu_rank_update(int terms, const HostTri& tri, Int m, Int n, double alpha, const Stor<T>* xr, Int incxr,
                     const Stor<T>* yc, Int incyc, const Stor<T>* yr, Int incyr,
                     const Stor<T>* xc, Int incxc, Stor<T>* A, Int lda) {
    using Cm = typename H<T>::C;
    for (Int j = 0; j < n; ++j) {
        const Cm sv = H<T>::ld(yc + j * incyc), tv = terms == 2 ? H<T>::ld(xc + j * incxc) : Cm(0);
        for (Int i = 0; i < m; ++i) {
            if (terms != 0 && !tri.in(i, j)) continue;
            Cm z = H<T>::ld(A + i + j * lda) + ((Cm)alpha * H<T>::ld(xr + i * incxr)) * sv;
            if (terms == 2) z += ((Cm)alpha * H<T>::ld(yr + i * incyr)) * tv;
            H<T>::st(A + i + j * lda, z);
        }
    }
}

}  // namespace exec
}  // namespace elx
