// "Run this with T bound to the element type of dtype code `t`", once for the
// launchers (.hip) and the host paths (.cpp).  `otherwise` is what an unknown
// code does: the launchers `return hipErrorInvalidValue`, exec throws.
#pragma once
#include "elem.hpp"
#include "../../../include/elemental_amd.h"

#define ELX_REAL_CASES(T, ...)                                                \
    case ELX_F64: { using T = double; __VA_ARGS__; break; }                   \
    case ELX_F32: { using T = float; __VA_ARGS__; break; }

// the routines that exist in f64 / f32 only
#define ELX_REAL_SWITCH(t, T, otherwise, ...)                                 \
    switch (static_cast<int>(t)) {                                            \
    ELX_REAL_CASES(T, __VA_ARGS__)                                            \
    default: otherwise;                                                       \
    }

#define ELX_DTYPE_SWITCH(t, T, otherwise, ...)                                \
    switch (static_cast<int>(t)) {                                            \
    ELX_REAL_CASES(T, __VA_ARGS__)                                            \
    case ELX_F16: { using T = ::elx::kern::f16_t; __VA_ARGS__; break; }       \
    case ELX_BF16: { using T = ::elx::kern::bf16_t; __VA_ARGS__; break; }     \
    default: otherwise;                                                       \
    }

// the launchers' form: an unknown code is an invalid argument
#define ELX_KERN_SWITCH(t, T, ...) ELX_DTYPE_SWITCH(t, T, return hipErrorInvalidValue, __VA_ARGS__)
#define ELX_KERN_REAL_SWITCH(t, T, ...) ELX_REAL_SWITCH(t, T, return hipErrorInvalidValue, __VA_ARGS__)

namespace elx {
namespace kern {

// bytes per element of a matrix dtype code; 0 for any other code
inline int dtype_size(int dtype) {
    ELX_DTYPE_SWITCH(dtype, T, return 0, return (int)sizeof(typename Elem<T>::storage));
    return 0;
}

}  // namespace kern
}  // namespace elx
