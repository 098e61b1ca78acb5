// Seed-stable stochastic sampling: the Philox4x32-10 normal generator (af_philox.h states the keying contract) and the fused
// DPM-Solver++(2M) SDE step.  A translation unit of its own: the kernels of af_elementwise.hip are not touched by it.
#include "../../include/adaface_hip.h"
#include "af_common.h"
#include "af_philox.h"
#include <cmath>

// ---------------------------------------------------------------------------------------------------------------------------
// af_philox_randn: out[s][e] = z(seed, id_s, stream, step, e), s < n_samples, e < per_sample.  One work item = one group of
// four elements of one sample; a 16-byte store when the output and per_sample allow it, else up to four scalar stores.
// ---------------------------------------------------------------------------------------------------------------------------
struct PhiloxRandnArgs {
  float* out;
  const long long* ids;   // NULL: first_id + s
  long long first_id;
  long n_samples, per_sample, gps;   // gps = groups per sample = ceil(per_sample / 4)
  unsigned long long seed;
  unsigned stream_id, step;
  int vec;                // out 16-byte aligned and per_sample % 4 == 0
};
__global__ void __launch_bounds__(128) philox_randn_kernel(const PhiloxRandnArgs a) {
  const long it = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (it >= a.n_samples * a.gps) return;
  const long s = it / a.gps, g = it - s * a.gps;
  const uint64_t id = (uint64_t)(a.ids ? a.ids[s] : a.first_id + s);
  float z[4];
  af_philox_normal4(a.seed, id, a.stream_id, a.step, (uint32_t)g, z);
  float* o = a.out + s * a.per_sample + 4 * g;
  if (a.vec) {
    *reinterpret_cast<float4*>(o) = make_float4(z[0], z[1], z[2], z[3]);
    return;
  }
  const long left = a.per_sample - 4 * g;   // >= 1
  o[0] = z[0];
  if (left > 1) o[1] = z[1];
  if (left > 2) o[2] = z[2];
  if (left > 3) o[3] = z[3];
}

// ---------------------------------------------------------------------------------------------------------------------------
// Fused classifier-free guidance + one DPM-Solver++(2M) SDE step (Lu et al. 2022, the "sde-dpmsolver++" multistep update of
// the authors' code), fp32, n elements:
//   e, x0, D as dpmpp_step_kernel (af_elementwise.hip);   x' = c_x x + c_d D + c_n z
//   c_x = (sigma_prev / sigma_t) e^-h, c_d = -alpha_prev expm1(-2h), c_n = sigma_prev sqrt(-expm1(-2h)): af_dpmpp_sde_coeffs
// z is generated in registers from the key (stream 1; NZ = false) or read from noise (NZ = true): no noise tensor is written.
// Every product-sum is an explicit fmaf, so the four-element path, the scalar path and the noise-pointer form give the same
// bits for an element.  fp32 roundings on an output's longest path, counted as if nothing were fused: x0_out 6 (3 without
// CFG) as dpmpp_step_kernel; D +2; c_d D, + c_x x, + c_n z: +3 => x_next 11 (9 / 8 / 6 without MS / CFG / both).  z carries
// the generator's own error (logf, sqrtf, sincospif, one product) into the last sum.
// Work items as dpmpp_step_kernel: four consecutive elements while it < n4, one element after that.  n4 > 0 only when every
// pointer is 16-byte aligned and, with in-kernel noise, per_sample % 4 == 0 (then a four-element item is one Philox group).
// Loads before the first use, stores after: x_next may be x.
// ---------------------------------------------------------------------------------------------------------------------------
struct DpmppSdeArgs {
  const float* x;
  const float* eps_c;
  const float* eps_u;
  const float* x0_prev;
  const float* noise;
  float* x_next;
  float* x0_out;
  long n, n4;
  float guidance, alpha_t, sigma_t, c_x, c_d, w_cur, w_prev, c_n;
  const long long* ids;
  long long first_id;
  long per_sample;
  unsigned long long seed;
  unsigned step;
};
template <bool CFG, bool MS>
__device__ __forceinline__ void dpmpp_sde_update(const DpmppSdeArgs& a, float xv, float ec, float eu, float xp, float z, float& xn,
                                                 float& p0) {
  float e = ec;
  if (CFG) e = fmaf(a.guidance, ec - eu, eu);
  p0 = fmaf(-a.sigma_t, e, xv) / a.alpha_t;
  float d = p0;
  if (MS) d = fmaf(a.w_cur, p0, a.w_prev * xp);
  xn = fmaf(a.c_n, z, fmaf(a.c_x, xv, a.c_d * d));
}
template <bool CFG, bool MS, bool NZ>
__global__ void __launch_bounds__(128) dpmpp_sde_step_kernel(const DpmppSdeArgs a) {
  const long it = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (it < a.n4) {
    const float4 xv = reinterpret_cast<const float4*>(a.x)[it];
    const float4 ec = reinterpret_cast<const float4*>(a.eps_c)[it];
    float4 eu = make_float4(0.f, 0.f, 0.f, 0.f), xp = eu;
    if (CFG) eu = reinterpret_cast<const float4*>(a.eps_u)[it];
    if (MS) xp = reinterpret_cast<const float4*>(a.x0_prev)[it];
    float z[4];
    if (NZ) {
      const float4 zv = reinterpret_cast<const float4*>(a.noise)[it];
      z[0] = zv.x; z[1] = zv.y; z[2] = zv.z; z[3] = zv.w;
    } else {
      const long i = 4 * it, s = i / a.per_sample, e0 = i - s * a.per_sample;   // per_sample % 4 == 0: e0 % 4 == 0
      const uint64_t id = (uint64_t)(a.ids ? a.ids[s] : a.first_id + s);
      af_philox_normal4(a.seed, id, AF_NOISE_STREAM_STEP, a.step, (uint32_t)(e0 >> 2), z);
    }
    float4 xn, p0;
    dpmpp_sde_update<CFG, MS>(a, xv.x, ec.x, eu.x, xp.x, z[0], xn.x, p0.x);
    dpmpp_sde_update<CFG, MS>(a, xv.y, ec.y, eu.y, xp.y, z[1], xn.y, p0.y);
    dpmpp_sde_update<CFG, MS>(a, xv.z, ec.z, eu.z, xp.z, z[2], xn.z, p0.z);
    dpmpp_sde_update<CFG, MS>(a, xv.w, ec.w, eu.w, xp.w, z[3], xn.w, p0.w);
    reinterpret_cast<float4*>(a.x_next)[it] = xn;
    if (a.x0_out) reinterpret_cast<float4*>(a.x0_out)[it] = p0;
    return;
  }
  const long i = 4 * a.n4 + (it - a.n4);
  if (i >= a.n) return;
  const float xv = a.x[i], ec = a.eps_c[i];
  float eu = 0.f, xp = 0.f, z;
  if (CFG) eu = a.eps_u[i];
  if (MS) xp = a.x0_prev[i];
  if (NZ) {
    z = a.noise[i];
  } else {
    const long s = i / a.per_sample, e = i - s * a.per_sample;
    const uint64_t id = (uint64_t)(a.ids ? a.ids[s] : a.first_id + s);
    z = af_philox_normal1(a.seed, id, AF_NOISE_STREAM_STEP, a.step, (uint64_t)e);
  }
  float xn, p0;
  dpmpp_sde_update<CFG, MS>(a, xv, ec, eu, xp, z, xn, p0);
  a.x_next[i] = xn;
  if (a.x0_out) a.x0_out[i] = p0;
}

template <bool CFG, bool MS>
static void launch_sde(bool nz, dim3 grid, dim3 block, hipStream_t s, const DpmppSdeArgs& a) {
  if (nz) hipLaunchKernelGGL((dpmpp_sde_step_kernel<CFG, MS, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((dpmpp_sde_step_kernel<CFG, MS, false>), grid, block, 0, s, a);
}

static const long kMaxPerSample = 4L << 32;   // the group index is one 32-bit counter word
static const unsigned kMaxStep = 1u << 24;

extern "C" {

int af_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  if (!ctr || !key || !out) { af_set_error_msg("af_philox4x32_10: null argument"); return AF_ERR_INVALID; }
  af_philox4x32_10_bits(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], out);
  return AF_OK;
}

int af_dpmpp_sde_coeffs(double acp_t, double acp_prev, double h_last, double out[9]) {
  // DPM-Solver++(2M) SDE on the schedule of af_dpmpp_coeffs.  The only place of the product that states these formulas.
  if (!out) { af_set_error_msg("af_dpmpp_sde_coeffs: null output"); return AF_ERR_INVALID; }
  if (!std::isfinite(acp_t) || !std::isfinite(acp_prev) || !std::isfinite(h_last)) {
    af_set_error_msg("af_dpmpp_sde_coeffs: non-finite argument (acp_t %g, acp_prev %g, h_last %g)", acp_t, acp_prev, h_last);
    return AF_ERR_INVALID;
  }
  if (!(acp_t > 0.0 && acp_t < 1.0 && acp_prev > 0.0 && acp_prev < 1.0)) {
    af_set_error_msg("af_dpmpp_sde_coeffs: acp_t %g / acp_prev %g outside (0, 1)", acp_t, acp_prev);
    return AF_ERR_INVALID;
  }
  if (!(acp_prev > acp_t)) {
    af_set_error_msg("af_dpmpp_sde_coeffs: acp_prev %g <= acp_t %g (a step must go towards less noise)", acp_prev, acp_t);
    return AF_ERR_INVALID;
  }
  const double alpha_t = sqrt(acp_t), sigma_t = sqrt(1.0 - acp_t);
  const double alpha_p = sqrt(acp_prev), sigma_p = sqrt(1.0 - acp_prev);
  // h as ONE logarithm (af_dpmpp_coeffs); 1 - e^-2h through expm1, which keeps its digits where h is small
  const double h = 0.5 * log((acp_prev * (1.0 - acp_t)) / (acp_t * (1.0 - acp_prev)));
  const double one_minus_e2h = -expm1(-2.0 * h);
  const bool second = h_last > 0.0;
  const double r = second ? h_last / h : 0.0;
  out[0] = alpha_t;
  out[1] = sigma_t;
  out[2] = (sigma_p / sigma_t) * exp(-h);
  out[3] = alpha_p * one_minus_e2h;
  out[4] = sigma_p * sqrt(one_minus_e2h);
  out[5] = second ? 1.0 + 1.0 / (2.0 * r) : 1.0;
  out[6] = second ? -1.0 / (2.0 * r) : 0.0;
  out[7] = h;
  out[8] = r;
  return AF_OK;
}

int af_philox_randn(float* out_dev, int64_t n_samples, int64_t per_sample, const int64_t* sample_ids_dev, int64_t first_id,
                    uint64_t seed, uint32_t stream_id, uint32_t step, void* stream) {
  if (!out_dev || n_samples <= 0 || per_sample <= 0) { af_set_error_msg("af_philox_randn: bad argument"); return AF_ERR_INVALID; }
  if (per_sample > kMaxPerSample || stream_id >= 256u || step >= kMaxStep || first_id < 0) {
    af_set_error_msg("af_philox_randn: per_sample %lld / stream %u / step %u / first_id %lld outside the keying contract "
                     "(per_sample <= 2^34, stream < 256, step < 2^24, id >= 0)", (long long)per_sample, stream_id, step,
                     (long long)first_id);
    return AF_ERR_INVALID;
  }
  PhiloxRandnArgs a{out_dev, reinterpret_cast<const long long*>(sample_ids_dev), (long long)first_id, (long)n_samples,
                    (long)per_sample, (long)((per_sample + 3) / 4), (unsigned long long)seed, stream_id, step,
                    (((uintptr_t)out_dev & 15) == 0 && per_sample % 4 == 0) ? 1 : 0};
  if (a.gps > 0x7fffffffL * 128 / a.n_samples) { af_set_error_msg("af_philox_randn: too large for one launch"); return AF_ERR_INVALID; }
  const long blocks = (a.n_samples * a.gps + 127) / 128;
  hipLaunchKernelGGL(philox_randn_kernel, dim3((unsigned)blocks), dim3(128), 0, reinterpret_cast<hipStream_t>(stream), a);
  HIP_CHECK_RET(hipGetLastError());
  return AF_OK;
}

int af_dpmpp_sde_step(const float* x_dev, const float* eps_cond_dev, const float* eps_uncond_dev, const float* x0_prev_dev, int64_t n,
                      float guidance, float alpha_t, float sigma_t, float c_x, float c_d, float w_cur, float w_prev,
                      float* x_next_dev, float* x0_out_dev, float c_n, const float* noise_dev, int64_t per_sample,
                      const int64_t* sample_ids_dev, int64_t first_id, uint64_t seed, uint32_t step, void* stream) {
  if (!x_dev || !eps_cond_dev || !x_next_dev || n <= 0) { af_set_error_msg("af_dpmpp_sde_step: bad argument"); return AF_ERR_INVALID; }
  if (!(alpha_t > 0.f)) { af_set_error_msg("af_dpmpp_sde_step: alpha_t %g is not positive", (double)alpha_t); return AF_ERR_INVALID; }
  if (!noise_dev && (per_sample <= 0 || per_sample > kMaxPerSample || n % per_sample != 0 || step >= kMaxStep || first_id < 0)) {
    af_set_error_msg("af_dpmpp_sde_step: n %lld / per_sample %lld / step %u / first_id %lld outside the keying contract "
                     "(n a multiple of per_sample <= 2^34, step < 2^24, id >= 0)", (long long)n, (long long)per_sample, step,
                     (long long)first_id);
    return AF_ERR_INVALID;
  }
  auto overlaps = [n](const float* p, const float* q) {
    return p && q && (uintptr_t)p < (uintptr_t)(q + n) && (uintptr_t)q < (uintptr_t)(p + n);
  };
  if (overlaps(x0_out_dev, x0_prev_dev) || overlaps(x0_out_dev, x_dev) || overlaps(x0_out_dev, x_next_dev)) {
    af_set_error_msg("af_dpmpp_sde_step: x0_out must not alias x0_prev, x or x_next");   // the rule of af_dpmpp_step
    return AF_ERR_INVALID;
  }
  // 16-byte path only when every pointer in use allows it, and a four-element item is one Philox group
  const uintptr_t bits = (uintptr_t)x_dev | (uintptr_t)eps_cond_dev | (uintptr_t)eps_uncond_dev | (uintptr_t)x0_prev_dev |
                         (uintptr_t)x_next_dev | (uintptr_t)x0_out_dev | (uintptr_t)noise_dev;
  const bool vec = (bits & 15) == 0 && (noise_dev || per_sample % 4 == 0);
  DpmppSdeArgs a{x_dev, eps_cond_dev, eps_uncond_dev, x0_prev_dev, noise_dev, x_next_dev, x0_out_dev, (long)n,
                 vec ? (long)(n / 4) : 0, guidance, alpha_t, sigma_t, c_x, c_d, w_cur, w_prev, c_n,
                 reinterpret_cast<const long long*>(sample_ids_dev), (long long)first_id, noise_dev ? 1 : (long)per_sample,
                 (unsigned long long)seed, step};
  const long items = a.n4 + (a.n - 4 * a.n4);
  const long blocks = (items + 127) / 128;
  if (blocks > 0x7fffffffL) { af_set_error_msg("af_dpmpp_sde_step: n = %lld is too large for one launch", (long long)n); return AF_ERR_INVALID; }
  const dim3 grid((unsigned)blocks), block(128);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool nz = noise_dev != nullptr;
  if (eps_uncond_dev && x0_prev_dev) launch_sde<true, true>(nz, grid, block, s, a);
  else if (eps_uncond_dev) launch_sde<true, false>(nz, grid, block, s, a);
  else if (x0_prev_dev) launch_sde<false, true>(nz, grid, block, s, a);
  else launch_sde<false, false>(nz, grid, block, s, a);
  HIP_CHECK_RET(hipGetLastError());
  return AF_OK;
}

}  // extern "C"
