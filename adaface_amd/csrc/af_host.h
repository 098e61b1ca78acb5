// Host-side helpers shared by the two host translation units, af_model.hip and af_ops.hip (and included by nothing else):
// error propagation, the per-dtype constants, where a LayerNorm consumer gets its row statistics from, and the one dtype
// dispatch.
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

// A LayerNorm-consumer launch whose row statistics are still the producer's partial sums `parts` [parts_n][p.M][2], once its
// plan is known: a kernel that keeps its rows for all of N (row-panel, 128 x 160 tile GEMM) is handed the partial sums and
// finalises (mu, rstd) of its rows in its prologue; any other reads them from `stats_buf` [p.M][2], which gets an
// ln_finalize launch here (none in a sizing pass, `dry`).  The caller planned with p.ln_stats = stats_buf.
static inline int af_ln_consumer_stats(ConvGemmParams& p, const AfGemmPlan& pl, const float* parts, int parts_n, int count,
                                       float eps, float* stats_buf, bool dry, hipStream_t s) {
  if (pl.kernel == AF_GK_ROWPANEL || pl.kernel == AF_GK_M128) {
    p.ln_stats = parts;
    p.ln_parts_n = parts_n;
    p.ln_inv_count = 1.0f / (float)count;
    p.ln_eps = eps;
    return 0;
  }
  p.ln_stats = stats_buf;
  return dry ? 0 : af_launch_ln_finalize(parts, parts_n, p.M, count, eps, stats_buf, s);
}

// f(AfTag<bf16 | f16 | float>{}) for the storage type of `dtype`: one argument list for the three instantiations of a launcher
template <typename T> struct AfTag { using type = T; };
template <typename F> static inline int af_dispatch(int dtype, F&& f) {
  return dtype == AF_DTYPE_BF16 ? f(AfTag<bf16>{}) : dtype == AF_DTYPE_F16 ? f(AfTag<f16>{}) : f(AfTag<float>{});
}
// AF_TYPED(dt, af_launch_silu<Elem>(p, p, n, s)): the expression with Elem = that storage type
#define AF_TYPED(dtype, ...) \
  af_dispatch((dtype), [&](auto af_tag_) { using Elem = typename decltype(af_tag_)::type; return (__VA_ARGS__); })
