// adaface_amd — img2img by strength and inpainting: the noising of a clean latent (Ho, Jain, Abbeel, "Denoising
// Diffusion Probabilistic Models", NeurIPS 2020, eq. 4; the start of SDEdit, Meng et al., ICLR 2022) and the known-region blend
// the latent-diffusion samplers run in front of every step (Lugmayr et al., "RePaint", CVPR 2022, eq. 8), in ONE launch:
//   z   = noise[b][e]  |  the Philox normal of (seed, id_b, stream, step, e)                  e = c HW + p
//   q   = fl( fl(sa x0) + fl(s1 z) )                              (s1 == 0: no noise is generated or read, q = fl(sa x0))
//   out = q  |  fl( fl(q m) + fl( fl(1 - m) x ) ),  m = keep[b][keep_channels == 1 ? 0 : c][p]
// fp32 NCHW latents.  It replaces the torch composition randn, q_sample (three element-wise launches) and
// img_orig * mask + (1. - mask) * img (four more), and gives its bits: every product and sum below is one fp32 operation rounded
// on its own.  The noise is the generator of af_philox.h under its one keying contract: the in-kernel z of an element is the
// bits af_philox_randn writes for it.
// Work items: four consecutive elements of one sample's one channel (one Philox group, one 16-byte access per operand) where
// every pointer is 16-byte aligned and HW % 4 == 0, one element otherwise.  An element's value is a function of its own
// operands and key alone, so both paths, every batch split and every launch size give the same bits for it.  Loads before the
// store of the same item, and no item reads what another writes: out may be x.
#include "../../include/adaface_hip.h"
#include "af_kernels.h"
#include "af_philox.h"

// No contraction in this file (as af_controlnet.hip): hipcc would turn sa * x0 + s1 * z into an fma, which rounds once where the
// composition this kernel replaces rounds twice.
#pragma clang fp contract(off)

std::atomic<long> g_af_noise_blend_launches{0};

namespace inpaint {

constexpr int kThreads = 256;
enum { NZ_NONE = 0, NZ_READ = 1, NZ_PHILOX = 2 };   // s1 == 0 / noise_dev / in-kernel generator

struct Args {
  const float* x;
  const float* x0;
  const float* keep;
  const float* noise;
  float* out;
  const long long* ids;     // NULL: first_id + b
  long long first_id;
  long n_samples, HW, per;  // per = C * HW, the sample length
  long items;               // vec: n_samples * per / 4, else n_samples * per
  int C, keep_full;         // keep_full: keep has C channels (else 1)
  float sa, s1;
  unsigned long long seed;
  unsigned stream_id, step;
};

// fl(fl(sa x0) + fl(s1 z)), then fl(fl(q m) + fl(fl(1 - m) x)): plain operators under the pragma above
template <int NZ, bool BLEND>
__device__ __forceinline__ float blend1(const Args& a, float x0, float z, float m, float x) {
  float q = a.sa * x0;
  if (NZ != NZ_NONE) {
    const float n = a.s1 * z;
    q = q + n;
  }
  if (!BLEND) return q;
  const float qm = q * m;
  const float om = 1.0f - m;
  const float xm = om * x;
  return qm + xm;
}

template <int NZ, bool BLEND, bool VEC>
__global__ __launch_bounds__(kThreads) void noise_blend_kernel(const Args a) {
  const long it = (long)blockIdx.x * kThreads + threadIdx.x;
  if (it >= a.items) return;
  const long i = VEC ? 4 * it : it;            // the item's first element in [n_samples][per]
  const long b = i / a.per, e = i - b * a.per;
  long ki = 0;
  if (BLEND) {
    ki = a.keep_full ? i : b * a.HW + e % a.HW;   // keep [n_samples][C | 1][HW]
  }
  uint64_t id = 0;
  if (NZ == NZ_PHILOX) id = (uint64_t)(a.ids ? a.ids[b] : a.first_id + b);
  if (VEC) {   // per % 4 == 0 and HW % 4 == 0: e % 4 == 0, the four elements are one Philox group of one channel
    const float4 v0 = *reinterpret_cast<const float4*>(a.x0 + i);
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (NZ == NZ_READ) {
      const float4 zv = *reinterpret_cast<const float4*>(a.noise + i);
      z[0] = zv.x; z[1] = zv.y; z[2] = zv.z; z[3] = zv.w;
    } else if (NZ == NZ_PHILOX) {
      af_philox_normal4(a.seed, id, a.stream_id, a.step, (uint32_t)(e >> 2), z);
    }
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f), xv = m;
    if (BLEND) {
      m = *reinterpret_cast<const float4*>(a.keep + ki);
      xv = *reinterpret_cast<const float4*>(a.x + i);
    }
    float4 o;
    o.x = blend1<NZ, BLEND>(a, v0.x, z[0], m.x, xv.x);
    o.y = blend1<NZ, BLEND>(a, v0.y, z[1], m.y, xv.y);
    o.z = blend1<NZ, BLEND>(a, v0.z, z[2], m.z, xv.z);
    o.w = blend1<NZ, BLEND>(a, v0.w, z[3], m.w, xv.w);
    *reinterpret_cast<float4*>(a.out + i) = o;
  } else {
    float z = 0.f;
    if (NZ == NZ_READ) z = a.noise[i];
    else if (NZ == NZ_PHILOX) z = af_philox_normal1(a.seed, id, a.stream_id, a.step, (uint64_t)e);
    float m = 0.f, xv = 0.f;
    if (BLEND) {
      m = a.keep[ki];
      xv = a.x[i];
    }
    a.out[i] = blend1<NZ, BLEND>(a, a.x0[i], z, m, xv);
  }
}

template <int NZ, bool BLEND>
static void launch(bool vec, dim3 grid, hipStream_t s, const Args& a) {
  if (vec) hipLaunchKernelGGL((noise_blend_kernel<NZ, BLEND, true>), grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL((noise_blend_kernel<NZ, BLEND, false>), grid, dim3(kThreads), 0, s, a);
}
template <int NZ>
static void launch_nz(bool blend, bool vec, dim3 grid, hipStream_t s, const Args& a) {
  if (blend) launch<NZ, true>(vec, grid, s, a);
  else launch<NZ, false>(vec, grid, s, a);
}

static const long kMaxPerSample = 4L << 32;   // the group index is one 32-bit counter word (af_philox.h)
static const unsigned kMaxStep = 1u << 24;

}  // namespace inpaint

extern "C" {

int64_t af_noise_blend_launches(void) { return (int64_t)g_af_noise_blend_launches.load(std::memory_order_relaxed); }

int af_noise_blend(const float* x_dev, const float* x0_dev, const float* keep_dev, int keep_channels, const float* noise_dev,
                   int64_t n_samples, int C, int64_t HW, float sa, float s1, const int64_t* sample_ids_dev, int64_t first_id,
                   uint64_t seed, uint32_t stream_id, uint32_t step, float* out_dev, void* stream) {
  using namespace inpaint;
  if (!x0_dev || !out_dev || n_samples <= 0 || C <= 0 || HW <= 0) {
    af_set_error_msg("af_noise_blend: bad argument (x0 %p, out %p, n_samples %lld, C %d, HW %lld)", (const void*)x0_dev,
                     (void*)out_dev, (long long)n_samples, C, (long long)HW);
    return AF_ERR_INVALID;
  }
  if (keep_channels != 1 && keep_channels != C) {
    af_set_error_msg("af_noise_blend: keep_channels %d is neither 1 nor C = %d", keep_channels, C);
    return AF_ERR_INVALID;
  }
  if (keep_dev && !x_dev) { af_set_error_msg("af_noise_blend: a keep mask without x (the latent to blend into)"); return AF_ERR_INVALID; }
  if (HW > kMaxPerSample / C) {
    af_set_error_msg("af_noise_blend: C %d x HW %lld is past the keying contract's sample length (2^34)", C, (long long)HW);
    return AF_ERR_INVALID;
  }
  const long per = (long)C * (long)HW;
  if (stream_id >= 256u || step >= kMaxStep || first_id < 0) {
    af_set_error_msg("af_noise_blend: stream %u / step %u / first_id %lld outside the keying contract (stream < 256, step < 2^24, "
                     "id >= 0)", stream_id, step, (long long)first_id);
    return AF_ERR_INVALID;
  }
  if (!(sa == sa) || sa - sa != 0.f || !(s1 == s1) || s1 - s1 != 0.f) {
    af_set_error_msg("af_noise_blend: sa %g / s1 %g is not finite", (double)sa, (double)s1);
    return AF_ERR_INVALID;
  }
  if (n_samples > 0x7fffffffL * (long)kThreads / per) {
    af_set_error_msg("af_noise_blend: %lld samples of %ld elements are too large for one launch", (long long)n_samples, per);
    return AF_ERR_INVALID;
  }
  const long n = (long)n_samples * per;
  const bool blend = keep_dev != nullptr;
  const int nz = s1 == 0.f ? NZ_NONE : (noise_dev ? NZ_READ : NZ_PHILOX);
  // out may be x exactly; it overlaps nothing else that the launch reads (bytes)
  auto overlaps = [](const void* p, long pb, const void* q, long qb) {
    return p && q && (uintptr_t)p < (uintptr_t)q + (uintptr_t)qb && (uintptr_t)q < (uintptr_t)p + (uintptr_t)pb;
  };
  const long nb = n * (long)sizeof(float);
  const long kb = (long)n_samples * keep_channels * (long)HW * (long)sizeof(float);
  if ((x_dev != out_dev && overlaps(out_dev, nb, x_dev, nb)) || overlaps(out_dev, nb, x0_dev, nb) ||
      overlaps(out_dev, nb, keep_dev, kb) || overlaps(out_dev, nb, noise_dev, nb) ||
      overlaps(out_dev, nb, sample_ids_dev, (long)n_samples * (long)sizeof(int64_t))) {
    af_set_error_msg("af_noise_blend: out overlaps an input (it may be x exactly, nothing else)");
    return AF_ERR_INVALID;
  }
  // 16-byte path only when every pointer the launch uses allows it and a four-element item is one Philox group of one channel
  uintptr_t bits = (uintptr_t)x0_dev | (uintptr_t)out_dev;
  if (blend) bits |= (uintptr_t)x_dev | (uintptr_t)keep_dev;
  if (nz == NZ_READ) bits |= (uintptr_t)noise_dev;
  const bool vec = (bits & 15) == 0 && HW % 4 == 0;
  Args a{blend ? x_dev : nullptr, x0_dev, keep_dev, nz == NZ_READ ? noise_dev : nullptr, out_dev,
         reinterpret_cast<const long long*>(sample_ids_dev), (long long)first_id, (long)n_samples, (long)HW, per,
         vec ? n / 4 : n, C, (blend && keep_channels == C && C != 1) ? 1 : 0, sa, s1, (unsigned long long)seed, stream_id, step};
  const long blocks = (a.items + kThreads - 1) / kThreads;
  const dim3 grid((unsigned)blocks);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // bytes moved: x0 and out always, z / keep / x where read
  const double bytes = (double)nb * (2.0 + (nz == NZ_READ ? 1.0 : 0.0) + (blend ? 1.0 : 0.0)) + (blend ? (double)kb : 0.0);
  AfProfScope prof(AF_K_NOISE_BLEND, s, 0.0, bytes);
  if (nz == NZ_NONE) launch_nz<NZ_NONE>(blend, vec, grid, s, a);
  else if (nz == NZ_READ) launch_nz<NZ_READ>(blend, vec, grid, s, a);
  else launch_nz<NZ_PHILOX>(blend, vec, grid, s, a);
  HIP_CHECK_RET(hipGetLastError());
  g_af_noise_blend_launches.fetch_add(1, std::memory_order_relaxed);
  return AF_OK;
}

}  // extern "C"
