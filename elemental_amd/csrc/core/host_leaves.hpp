// Device::CPU, the factorisation leaves: the unblocked loops behind
// exec::Cholesky, LU, Laswp, QR (and its three helpers), HostHermitianTridiag,
// TriangularInverse and Trtrmm.  f64 / f32 only, computed in the element type itself.
#pragma once
#include "../common.hpp"
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

namespace elx {
namespace exec {

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

template <typename S>
void cpu_laswp(Int m, Int n, S* A, Int lda, const int* piv, Int k0, Int k1, Int voff, bool inverse) {
    for (Int q = k0; q < k1; ++q) {
        const Int k = inverse ? k0 + k1 - 1 - q : q, p = (Int)piv[k] - voff;
        if (p == k || p < 0 || p >= m || k >= m) continue;
        for (Int c = 0; c < n; ++c) std::swap(A[k + c * lda], A[p + c * lda]);
    }
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

template <typename S>
void cpu_qr_explicit_u(Int m, Int nb, const S* A, Int lda, S* U, Int ldu, bool upper, Int off) {
    for (Int c = 0; c < nb; ++c)
        for (Int i = 0; i < m; ++i) {
            const Int d = off + c;
            U[i + c * ldu] = (upper ? i < d : i > d) ? A[i + c * lda] : (i == d ? S(1) : S(0));
        }
}

// The unblocked tridiagonalization (the sequential loop of herm_tridiag::
// LowerBlocked / UpperBlocked) with cpu_qr_panel's reflector.  S(i,j), i >= j, is
// A(i,j) when lower; when upper it is A(n-1-i, n-1-j): UPPER is LOWER on the
// matrix with both index orders reversed, and tau is reversed with it.  Per
// column k: the reflector of S(k+1:n, k) (pivot row k+1), w = t S22 v, w -=
// (t/2)(w.v) v, S22 -= v w^T + w v^T on the stored triangle.  Sums in double
template <typename S>
void cpu_sytrd(bool lower, Int n, S* A, Int lda, S* tau) {
    auto a = [&](Int i, Int j) -> S& { return lower ? A[i + j * lda] : A[(n - 1 - i) + (n - 1 - j) * lda]; };
    std::vector<double> v(n > 0 ? n : 0), w(n > 0 ? n : 0);
    for (Int k = 0; k + 1 < n; ++k) {
        double mx = 0.0;
        for (Int i = k + 2; i < n; ++i) {
            const double x = std::fabs((double)a(i, k));
            if (x > mx || x != x) mx = x;  // a NaN stays
        }
        const double alpha = (double)a(k + 1, k);
        double beta, t;
        if (mx == 0.0) {
            beta = -alpha;
            t = 2.0;
            for (Int i = k + 2; i < n; ++i) a(i, k) = S(0);
        } else {
            double ssq = 0.0;
            for (Int i = k + 2; i < n; ++i) {
                const double r = (double)a(i, k) / mx;
                ssq += r * r;
            }
            const double nrm = std::hypot(alpha, mx * std::sqrt(ssq));
            beta = alpha <= 0.0 ? nrm : -nrm;
            t = (double)(S)((beta - alpha) / beta);
            const double denom = alpha - beta;
            for (Int i = k + 2; i < n; ++i) a(i, k) = (S)((double)a(i, k) / denom);
        }
        v[k + 1] = 1.0;
        for (Int i = k + 2; i < n; ++i) v[i] = (double)a(i, k);
        for (Int i = k + 1; i < n; ++i) w[i] = 0.0;
        for (Int j = k + 1; j < n; ++j) {
            w[j] += (double)a(j, j) * v[j];
            for (Int i = j + 1; i < n; ++i) {
                const double x = (double)a(i, j);
                w[i] += x * v[j];
                w[j] += x * v[i];
            }
        }
        double dot = 0.0;
        for (Int i = k + 1; i < n; ++i) {
            w[i] *= t;
            dot += w[i] * v[i];
        }
        const double coef = -0.5 * t * dot;
        for (Int i = k + 1; i < n; ++i) w[i] = (double)(S)(w[i] + coef * v[i]);
        for (Int j = k + 1; j < n; ++j)
            for (Int i = j; i < n; ++i) a(i, j) = (S)((double)a(i, j) - (v[i] * w[j] + w[i] * v[j]));
        a(k + 1, k) = (S)beta;
        tau[lower ? k : n - 2 - k] = (S)t;
    }
}

template <typename S>
void cpu_qr_fix_t(Int nb, S* T, Int ldt, const S* tau) {
    for (Int c = 0; c < nb; ++c) {
        for (Int i = 0; i < c; ++i) T[i + c * ldt] = S(0);
        T[c + c * ldt] = S(1) / tau[c];
    }
}

template <typename S>
void cpu_row_scale(Int m, Int n, S* A, Int lda, const S* sig, Int i0, Int is) {
    for (Int c = 0; c < n; ++c)
        for (Int i = 0; i < m; ++i) A[i + c * lda] *= sig[i0 + i * is];
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

}  // namespace exec
}  // namespace elx
