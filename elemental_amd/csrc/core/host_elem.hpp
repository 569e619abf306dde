// Device::CPU, elementwise: the host view of one element and the loops of
// exec.cpp that go entry by entry.  Pure templates, no HIP runtime calls.
#pragma once
#include "../common.hpp"
#include "../kernels/dtype_switch.hpp"
#include "../kernels/kernels.hpp"
#include <cmath>
#include <type_traits>

namespace elx {
namespace exec {

// Host element access by pointer in the compute type of T (f16/bf16 -> float),
// over the kernels' Elem<T>.  The f16 store goes through FloatToHalf: the two
// agree on every float that is not a NaN, but FloatToHalf stores the canonical
// sign | 0x7e00 where Elem<f16_t>::store (a _Float16 cast) keeps payload bits;
// they differ on 16 744 448 of the NaN inputs, and the host paths store the
// canonical one.
template <typename T>
struct H {
    using S = typename kern::Elem<T>::storage;
    using C = typename kern::Elem<T>::compute;
    static C ld(const S* p) { return kern::Elem<T>::load(*p); }
    static void st(S* p, C v) {
        if constexpr (std::is_same<T, kern::f16_t>::value) *p = FloatToHalf(v);
        else *p = kern::Elem<T>::store(v);
    }
};
template <typename T> using Stor = typename H<T>::S;

template <typename T>
void cpu_copy(const kern::Copy2D& d, bool axpy, double alpha) {
    using S = typename H<T>::S;
    using C = typename H<T>::C;
    const S* src = static_cast<const S*>(d.src);
    S* dst = static_cast<S*>(d.dst);
    const C a = (C)alpha;
    for (Int j = 0; j < d.n; ++j)
        for (Int i = 0; i < d.m; ++i) {
            const S* x = src + i * d.scs + j * d.srs;
            S* y = dst + i * d.dcs + j * d.drs;
            if (axpy) H<T>::st(y, H<T>::ld(y) + a * H<T>::ld(x));
            else *y = *x;
        }
}

// what kern::convert_elem stores, a NaN included
template <typename TS, typename TD>
void cpu_convert(const kern::Copy2D& d) {
    using SS = typename kern::Elem<TS>::storage;
    using SD = typename kern::Elem<TD>::storage;
    const SS* src = static_cast<const SS*>(d.src);
    SD* dst = static_cast<SD*>(d.dst);
    for (Int j = 0; j < d.n; ++j)
        for (Int i = 0; i < d.m; ++i)
            dst[i * d.dcs + j * d.drs] = kern::convert_elem<TS, TD>(src[i * d.scs + j * d.srs]);
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

}  // namespace exec
}  // namespace elx
