// adaface_amd — few-step sampling with consistency models: the per-step scalars of the LCM update (Luo, Tan, Huang,
// Li, Zhao, "Latent Consistency Models", 2023, Algorithm 3 with the boundary condition of Song et al., "Consistency Models",
// ICML 2023, section 3) and of TCD's strategic stochastic sampling (Zheng et al., "Trajectory Consistency Distillation", 2024,
// Algorithm 4), and the ONE launch that performs a step.  A translation unit of its own: the kernels of af_philox.hip and
// af_elementwise.hip are not touched by it; the noise is af_philox.h's generator under its one keying contract.
#include "../../include/adaface_hip.h"
#include "af_kernels.h"
#include "af_philox.h"
#include <cmath>

std::atomic<long> g_af_lcm_step_launches{0};

// ---------------------------------------------------------------------------------------------------------------------------
// Fused classifier-free guidance + one consistency step, fp32, n elements:
//   e  = e_u + g (e_c - e_u)                                  (CFG; without e_u: e = e_c)
//   x0 = (x - sigma_t e) / alpha_t
//   D  = k_out x0 + k_skip x                 -> d_out         (the denoised sample: what callbacks see as pred_x0)
//   x' = c_x x + c_0 x0 + c_n z              -> x_next        (c_n == 0: no z is read or generated)
// with (k_out, k_skip, c_x, c_0, c_n) from af_lcm_coeffs.  z is read from noise (NZ_READ) or generated in registers from the key
// (stream 1, NZ_PHILOX): the bits af_philox_randn writes for that element; no noise tensor is written.
// Every product-sum is an explicit fmaf, so the four-element path, the scalar path and the three noise forms give the same bits
// for an element wherever they compute the same terms.  fp32 roundings on an output's longest path, counted as if nothing
// were fused:
//   e      sub, mul, add                     3      (no CFG: 0)
//   x0     mul, sub, IEEE division          +3  =>  x0: 6 (3 without CFG)
//   D      k_out x0, + k_skip x             +2  =>  d_out: 8 (5)          (k_skip x is rounded once, off the longest path)
//   x'     c_0 x0, + c_x x, + c_n z         +3  =>  x_next: 9 (6);  c_n == 0: +2 => 8 (5)
// z carries the generator's own error (logf, sqrtf, sincospif, one product) into the last sum.
// Work items as dpmpp_sde_step_kernel: four consecutive elements while it < n4, one element after that.  n4 > 0 only when every
// pointer in use is 16-byte aligned and, with in-kernel noise, per_sample % 4 == 0 (then a four-element item is one Philox
// group).  Loads before the first use, stores after: x_next may be x.  d_out aliases no input (af_lcm_step refuses it).
// Instantiated on (CFG, noise source) alone: the coefficients are arguments, never template parameters.
// ---------------------------------------------------------------------------------------------------------------------------
namespace lcm {

enum { NZ_NONE = 0, NZ_READ = 1, NZ_PHILOX = 2 };   // c_n == 0 / noise_dev / in-kernel generator

struct Args {
  const float* x;
  const float* eps_c;
  const float* eps_u;
  const float* noise;
  float* x_next;
  float* d_out;
  long n, n4;
  float guidance, alpha_t, sigma_t, k_out, k_skip, c_x, c_0, c_n;
  const long long* ids;   // NULL: first_id + s
  long long first_id;
  long per_sample;
  unsigned long long seed;
  unsigned step;
};

template <bool CFG, int NZ>
__device__ __forceinline__ void update(const Args& a, float xv, float ec, float eu, float z, float& xn, float& d) {
  float e = ec;
  if (CFG) e = fmaf(a.guidance, ec - eu, eu);
  const float p0 = fmaf(-a.sigma_t, e, xv) / a.alpha_t;
  d = fmaf(a.k_out, p0, a.k_skip * xv);
  xn = fmaf(a.c_x, xv, a.c_0 * p0);
  if (NZ != NZ_NONE) xn = fmaf(a.c_n, z, xn);
}

template <bool CFG, int NZ>
__global__ void __launch_bounds__(128) lcm_step_kernel(const Args a) {
  const long it = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (it < a.n4) {
    const float4 xv = reinterpret_cast<const float4*>(a.x)[it];
    const float4 ec = reinterpret_cast<const float4*>(a.eps_c)[it];
    float4 eu = make_float4(0.f, 0.f, 0.f, 0.f);
    if (CFG) eu = reinterpret_cast<const float4*>(a.eps_u)[it];
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (NZ == NZ_READ) {
      const float4 zv = reinterpret_cast<const float4*>(a.noise)[it];
      z[0] = zv.x; z[1] = zv.y; z[2] = zv.z; z[3] = zv.w;
    } else if (NZ == NZ_PHILOX) {
      const long i = 4 * it, s = i / a.per_sample, e0 = i - s * a.per_sample;   // per_sample % 4 == 0: e0 % 4 == 0
      const uint64_t id = (uint64_t)(a.ids ? a.ids[s] : a.first_id + s);
      af_philox_normal4(a.seed, id, AF_NOISE_STREAM_STEP, a.step, (uint32_t)(e0 >> 2), z);
    }
    float4 xn, d;
    update<CFG, NZ>(a, xv.x, ec.x, eu.x, z[0], xn.x, d.x);
    update<CFG, NZ>(a, xv.y, ec.y, eu.y, z[1], xn.y, d.y);
    update<CFG, NZ>(a, xv.z, ec.z, eu.z, z[2], xn.z, d.z);
    update<CFG, NZ>(a, xv.w, ec.w, eu.w, z[3], xn.w, d.w);
    reinterpret_cast<float4*>(a.x_next)[it] = xn;
    if (a.d_out) reinterpret_cast<float4*>(a.d_out)[it] = d;
    return;
  }
  const long i = 4 * a.n4 + (it - a.n4);
  if (i >= a.n) return;
  const float xv = a.x[i], ec = a.eps_c[i];
  float eu = 0.f, z = 0.f;
  if (CFG) eu = a.eps_u[i];
  if (NZ == NZ_READ) {
    z = a.noise[i];
  } else if (NZ == NZ_PHILOX) {
    const long s = i / a.per_sample, e = i - s * a.per_sample;
    const uint64_t id = (uint64_t)(a.ids ? a.ids[s] : a.first_id + s);
    z = af_philox_normal1(a.seed, id, AF_NOISE_STREAM_STEP, a.step, (uint64_t)e);
  }
  float xn, d;
  update<CFG, NZ>(a, xv, ec, eu, z, xn, d);
  a.x_next[i] = xn;
  if (a.d_out) a.d_out[i] = d;
}

template <bool CFG>
static void launch(int nz, dim3 grid, dim3 block, hipStream_t s, const Args& a) {
  if (nz == NZ_NONE) hipLaunchKernelGGL((lcm_step_kernel<CFG, NZ_NONE>), grid, block, 0, s, a);
  else if (nz == NZ_READ) hipLaunchKernelGGL((lcm_step_kernel<CFG, NZ_READ>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((lcm_step_kernel<CFG, NZ_PHILOX>), grid, block, 0, s, a);
}

static const long kMaxPerSample = 4L << 32;   // the group index is one 32-bit counter word (af_philox.h)
static const unsigned kMaxStep = 1u << 24;

}  // namespace lcm

extern "C" {

int64_t af_lcm_step_launches(void) { return (int64_t)g_af_lcm_step_launches.load(std::memory_order_relaxed); }

int af_lcm_coeffs(double acp_t, double acp_prev, double acp_s, int64_t t, double timestep_scaling, double sigma_data,
                  double out[7]) {
  // The only place of the product that states these formulas.  x0 = (x - sigma e) / alpha; the step is x' = c_x x + c_0 x0 + c_n z.
  if (!out) { af_set_error_msg("af_lcm_coeffs: null output"); return AF_ERR_INVALID; }
  if (!std::isfinite(acp_t) || !std::isfinite(acp_prev) || !std::isfinite(acp_s) || !std::isfinite(timestep_scaling) ||
      !std::isfinite(sigma_data)) {
    af_set_error_msg("af_lcm_coeffs: non-finite argument (acp_t %g, acp_prev %g, acp_s %g, timestep_scaling %g, sigma_data %g)",
                     acp_t, acp_prev, acp_s, timestep_scaling, sigma_data);
    return AF_ERR_INVALID;
  }
  const bool tcd = acp_s > 0.0;
  if (!(acp_t > 0.0 && acp_t <= 1.0 && acp_prev > 0.0 && acp_prev <= 1.0 && acp_s <= 1.0)) {
    af_set_error_msg("af_lcm_coeffs: acp_t %g / acp_prev %g / acp_s %g outside (0, 1]", acp_t, acp_prev, acp_s);
    return AF_ERR_INVALID;
  }
  if (!(acp_prev > acp_t)) {
    af_set_error_msg("af_lcm_coeffs: acp_prev %g <= acp_t %g (a step must go towards less noise)", acp_prev, acp_t);
    return AF_ERR_INVALID;
  }
  if (tcd && !(acp_prev <= acp_s)) {
    af_set_error_msg("af_lcm_coeffs: TCD needs acp_t <= acp_prev <= acp_s, got acp_prev %g > acp_s %g (the intermediate timestep "
                     "s lies at or below the next one)", acp_prev, acp_s);
    return AF_ERR_INVALID;
  }
  if (t < 0 || !(timestep_scaling > 0.0) || !(sigma_data > 0.0)) {
    af_set_error_msg("af_lcm_coeffs: timestep %lld / timestep_scaling %g / sigma_data %g: t >= 0 and positive scales expected",
                     (long long)t, timestep_scaling, sigma_data);
    return AF_ERR_INVALID;
  }
  const double alpha_t = sqrt(acp_t), sigma_t = sqrt(1.0 - acp_t);
  const bool final_step = acp_prev == 1.0;
  double k_out = 1.0, k_skip = 0.0, c_x, c_0, c_n;
  if (!tcd) {
    // the boundary condition of the consistency function: f(x, t) = c_skip(t) x + c_out(t) x0, c_skip(0) = 1, c_out(0) = 0
    const double tau = (double)t * timestep_scaling, sd2 = sigma_data * sigma_data;
    k_skip = sd2 / (tau * tau + sd2);
    k_out = tau / sqrt(tau * tau + sd2);
    const double a_p = sqrt(acp_prev);
    c_x = a_p * k_skip;            // x' = sqrt(acp_prev) D + sqrt(1 - acp_prev) z
    c_0 = a_p * k_out;
    c_n = sqrt(1.0 - acp_prev);
  } else {
    // D = x0;  pn = sqrt(acp_s) x0 + sqrt(1 - acp_s) e with e = (x - alpha x0) / sigma;  x' = r pn + sqrt(1 - r^2) z
    const double r2 = acp_prev / acp_s, r = sqrt(r2), sig_s = sqrt(1.0 - acp_s);
    c_x = r * sig_s / sigma_t;
    c_0 = r * (sqrt(acp_s) - alpha_t * sig_s / sigma_t);
    c_n = sqrt(1.0 - r2);
  }
  if (final_step) {   // both modes: the run returns the denoised sample
    c_x = k_skip;
    c_0 = k_out;
    c_n = 0.0;
  }
  out[0] = alpha_t;
  out[1] = sigma_t;
  out[2] = k_out;
  out[3] = k_skip;
  out[4] = c_x;
  out[5] = c_0;
  out[6] = c_n;
  return AF_OK;
}

int af_lcm_step(const float* x_dev, const float* eps_cond_dev, const float* eps_uncond_dev, int64_t n, float guidance, float alpha_t,
                float sigma_t, float k_out, float k_skip, float c_x, float c_0, float c_n, float* x_next_dev, float* d_out_dev,
                const float* noise_dev, int64_t per_sample, const int64_t* sample_ids_dev, int64_t first_id, uint64_t seed,
                uint32_t step, void* stream) {
  using namespace lcm;
  if (!x_dev || !eps_cond_dev || !x_next_dev || n <= 0) { af_set_error_msg("af_lcm_step: bad argument"); return AF_ERR_INVALID; }
  if (!(alpha_t > 0.f)) { af_set_error_msg("af_lcm_step: alpha_t %g is not positive", (double)alpha_t); return AF_ERR_INVALID; }
  const int nz = c_n == 0.f ? NZ_NONE : (noise_dev ? NZ_READ : NZ_PHILOX);
  if (nz == NZ_PHILOX && (per_sample <= 0 || per_sample > kMaxPerSample || n % per_sample != 0 || step >= kMaxStep || first_id < 0)) {
    af_set_error_msg("af_lcm_step: n %lld / per_sample %lld / step %u / first_id %lld outside the keying contract "
                     "(n a multiple of per_sample <= 2^34, step < 2^24, id >= 0)", (long long)n, (long long)per_sample, step,
                     (long long)first_id);
    return AF_ERR_INVALID;
  }
  auto overlaps = [n](const float* p, const float* q) {
    return p && q && (uintptr_t)p < (uintptr_t)(q + n) && (uintptr_t)q < (uintptr_t)(p + n);
  };
  if (overlaps(d_out_dev, x_dev) || overlaps(d_out_dev, x_next_dev)) {
    af_set_error_msg("af_lcm_step: d_out must not alias x or x_next");
    return AF_ERR_INVALID;
  }
  // 16-byte path only when every pointer in use allows it, and a four-element item is one Philox group
  uintptr_t bits = (uintptr_t)x_dev | (uintptr_t)eps_cond_dev | (uintptr_t)eps_uncond_dev | (uintptr_t)x_next_dev |
                   (uintptr_t)d_out_dev;
  if (nz == NZ_READ) bits |= (uintptr_t)noise_dev;
  const bool vec = (bits & 15) == 0 && (nz != NZ_PHILOX || per_sample % 4 == 0);
  Args a{x_dev, eps_cond_dev, eps_uncond_dev, nz == NZ_READ ? noise_dev : nullptr, x_next_dev, d_out_dev, (long)n,
         vec ? (long)(n / 4) : 0, guidance, alpha_t, sigma_t, k_out, k_skip, c_x, c_0, c_n,
         reinterpret_cast<const long long*>(sample_ids_dev), (long long)first_id, nz == NZ_PHILOX ? (long)per_sample : 1,
         (unsigned long long)seed, step};
  const long items = a.n4 + (a.n - 4 * a.n4);
  const long blocks = (items + 127) / 128;
  if (blocks > 0x7fffffffL) { af_set_error_msg("af_lcm_step: n = %lld is too large for one launch", (long long)n); return AF_ERR_INVALID; }
  const dim3 grid((unsigned)blocks), block(128);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (eps_uncond_dev) launch<true>(nz, grid, block, s, a);
  else launch<false>(nz, grid, block, s, a);
  HIP_CHECK_RET(hipGetLastError());
  g_af_lcm_step_launches.fetch_add(1, std::memory_order_relaxed);
  return AF_OK;
}

}  // extern "C"
