// adaface_amd — T-GATE: Zhang et al., "Cross-Attention Makes Inference Cumbersome in Text-to-Image Diffusion Models"
// (2024).  After the gate step the cross-attention outputs are frozen, averaged over the guidance legs, and the U-Net runs on one
// leg.  One kernel serves both phases of a cross-attention site:
//   capture  src = o [L B][N][C], attn2's output (to_out + bias) without its residual:
//              A[b]         = round(mean over the L legs of o[l B + b])     -> cache (fp32 sum, x 0.5 for L = 2, rounded once)
//              t2[l B + b]  = round(t1[l B + b] + o[l B + b])               for every leg
//   replay   src = A [B][N][C], L = 1, no cache output:  t2[b] = round(t1[b] + A[b])
// and, optionally, the LayerNorm row sums of t2 in the layout of ConvGemmParams::ln_stats_out ([parts][rows][2], af_common.h):
// the sum and the sum of squares of the ROUNDED values of every row, whole row in part 0 and zeros in the other parts -- the
// consumers add the parts up (as tome_unmerge_add_kernel leaves them).
// One wave per row of a sample b (and its L legs): the row sums are a cross-lane reduction, nothing is atomic, the order of the
// additions is fixed.  Every vector of a row is loaded from all of its sources before anything is stored, so t2 may be src.
#include "af_kernels.h"

namespace tgate {

template <typename T, bool VEC, int L>
__global__ __launch_bounds__(256) void tgate_add_kernel(const T* __restrict__ t1, int ld1, const T* src, int lds, T* t2, int ld2,
                                                        T* __restrict__ cache, int ldc, long rows_leg, int Cn,
                                                        float* __restrict__ stats, int parts) {
  constexpr int EPC = VEC ? 16 / (int)sizeof(T) : 1;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows_leg) return;
  const int NV = Cn / EPC;
  float s1[L], s2[L];
#pragma unroll
  for (int l = 0; l < L; ++l) s1[l] = s2[l] = 0.f;
  for (int vi = lane; vi < NV; vi += 64) {
    float o[L][EPC], r[L][EPC];
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const long rl = (long)l * rows_leg + row;
      if constexpr (VEC) {
        Vec16<T> a, b;
        a.u = *reinterpret_cast<const uint4*>(src + rl * lds + vi * EPC);
        b.u = *reinterpret_cast<const uint4*>(t1 + rl * ld1 + vi * EPC);
#pragma unroll
        for (int e = 0; e < EPC; ++e) { o[l][e] = to_f32<T>(a.e[e]); r[l][e] = to_f32<T>(b.e[e]); }
      } else {
        o[l][0] = to_f32<T>(src[rl * lds + vi]);
        r[l][0] = to_f32<T>(t1[rl * ld1 + vi]);
      }
    }
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const long rl = (long)l * rows_leg + row;
      T out[EPC];
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        out[e] = from_f32<T>(r[l][e] + o[l][e]);
        const float f = to_f32<T>(out[e]);
        s1[l] += f;
        s2[l] += f * f;
      }
      if constexpr (VEC) {
        Vec16<T> w;
#pragma unroll
        for (int e = 0; e < EPC; ++e) w.e[e] = out[e];
        *reinterpret_cast<uint4*>(t2 + rl * ld2 + vi * EPC) = w.u;
      } else {
        t2[rl * ld2 + vi] = out[0];
      }
    }
    if (cache) {
      T m[EPC];
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        if constexpr (L == 2) m[e] = from_f32<T>((o[0][e] + o[1][e]) * 0.5f);
        else m[e] = from_f32<T>(o[0][e]);
      }
      if constexpr (VEC) {
        Vec16<T> w;
#pragma unroll
        for (int e = 0; e < EPC; ++e) w.e[e] = m[e];
        *reinterpret_cast<uint4*>(cache + row * ldc + vi * EPC) = w.u;
      } else {
        cache[row * ldc + vi] = m[0];
      }
    }
  }
  if (stats) {
    const long rows = (long)L * rows_leg;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      float a = s1[l], b = s2[l];
#pragma unroll
      for (int sh = 32; sh > 0; sh >>= 1) {
        a += __shfl_xor(a, sh, 64);
        b += __shfl_xor(b, sh, 64);
      }
      const long rl = (long)l * rows_leg + row;
      for (int p = lane; p < parts; p += 64) {
        float* d = stats + ((long)p * rows + rl) * 2;
        d[0] = p == 0 ? a : 0.f;
        d[1] = p == 0 ? b : 0.f;
      }
    }
  }
}

}  // namespace tgate

template <typename T>
int af_launch_tgate_add(const void* t1, int ld1, const void* src, int lds, void* t2, int ld2, void* cache, int ldc, int L, int B,
                        int N, int C, float* ln_stats_out, int ln_parts, hipStream_t s) {
  constexpr int EPC = 16 / (int)sizeof(T);
  if (L != 1 && L != 2) { af_set_error_msg("tgate add: %d legs (1 or 2)", L); return -1; }
  if (B < 0 || N <= 0 || C <= 0) { af_set_error_msg("tgate add: bad shape B=%d N=%d C=%d", B, N, C); return -1; }
  if (!t1 || !src || !t2) { af_set_error_msg("tgate add: null operand"); return -1; }
  if (ld1 < C || lds < C || ld2 < C || (cache && ldc < C)) { af_set_error_msg("tgate add: a row stride is below C=%d", C); return -1; }
  if (ln_stats_out && ln_parts <= 0) { af_set_error_msg("tgate add: LayerNorm statistics without a part count"); return -1; }
  if (B == 0) return 0;
  const long rows_leg = (long)B * N;
  if ((rows_leg + 3) / 4 > 0x7fffffffL) { af_set_error_msg("tgate add: %ld rows exceed one launch", rows_leg); return -1; }
  auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool vec = C % EPC == 0 && ld1 % EPC == 0 && lds % EPC == 0 && ld2 % EPC == 0 && al(t1) && al(src) && al(t2) &&
                   (!cache || (ldc % EPC == 0 && al(cache)));
  AfProfScope prof(AF_K_TGATE_ADD, s, 0.0, (double)rows_leg * C * sizeof(T) * (3.0 * L + (cache ? 1.0 : 0.0)));
  const dim3 grid((unsigned)((rows_leg + 3) / 4)), block(256);
  const T* a = reinterpret_cast<const T*>(t1);
  const T* b = reinterpret_cast<const T*>(src);
  T* y = reinterpret_cast<T*>(t2);
  T* c = reinterpret_cast<T*>(cache);
#define AF_TGATE_LAUNCH(V, LL) \
  hipLaunchKernelGGL((tgate::tgate_add_kernel<T, V, LL>), grid, block, 0, s, a, ld1, b, lds, y, ld2, c, ldc, rows_leg, C, ln_stats_out, ln_parts)
  if (vec) { if (L == 2) AF_TGATE_LAUNCH(true, 2); else AF_TGATE_LAUNCH(true, 1); }
  else { if (L == 2) AF_TGATE_LAUNCH(false, 2); else AF_TGATE_LAUNCH(false, 1); }
#undef AF_TGATE_LAUNCH
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

#define AF_TGATE_INST(T) \
  template int af_launch_tgate_add<T>(const void*, int, const void*, int, void*, int, void*, int, int, int, int, int, float*, int, hipStream_t);
AF_TGATE_INST(bf16)
AF_TGATE_INST(f16)
AF_TGATE_INST(float)
