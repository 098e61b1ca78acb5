// Host-side helpers shared by the two host translation units, af_model.hip and af_ops.hip (and included by nothing else):
// error propagation, the per-dtype constants and the one dtype dispatch.
#pragma once
#include "af_kernels.h"

#define AF_TRY(expr)            \
  do {                          \
    int _rc = (expr);           \
    if (_rc != 0) return _rc;   \
  } while (0)

static inline size_t esize(int dtype) { return dtype == AF_DTYPE_F32 ? 4 : 2; }
static inline int bk_of(int dtype) { return dtype == AF_DTYPE_F32 ? 32 : 64; }
// the planner's name for a handle's storage type
static inline AfStorage storage_of(int dtype) { return dtype == AF_DTYPE_BF16 ? AF_ST_BF16 : dtype == AF_DTYPE_F16 ? AF_ST_F16 : AF_ST_F32; }
static inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// f(AfTag<bf16 | f16 | float>{}) for the storage type of `dtype`: one argument list for the three instantiations of a launcher
template <typename T> struct AfTag { using type = T; };
template <typename F> static inline int af_dispatch(int dtype, F&& f) {
  return dtype == AF_DTYPE_BF16 ? f(AfTag<bf16>{}) : dtype == AF_DTYPE_F16 ? f(AfTag<f16>{}) : f(AfTag<float>{});
}
// AF_TYPED(dt, af_launch_silu<Elem>(p, p, n, s)): the expression with Elem = that storage type
#define AF_TYPED(dtype, ...) \
  af_dispatch((dtype), [&](auto af_tag_) { using Elem = typename decltype(af_tag_)::type; return (__VA_ARGS__); })
