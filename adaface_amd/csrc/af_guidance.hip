// adaface_amd — the guidance combine of a sampler step with perturbed-attention guidance (Ahn et al., "Self-Rectifying Diffusion
// Sampling with Perturbed-Attention Guidance", ECCV 2024) and guidance rescale (Lin et al., "Common Diffusion Noise Schedules and
// Sample Steps are Flawed", WACV 2024, section 3.4; diffusers' rescale_noise_cfg), fp32, n_samples samples of per_sample elements:
//
//   e   = e_u + w (e_c - e_u) + s (e_c - e_p)          (e_p NULL or s = 0: no s term; e_u NULL: e = e_c + s (e_c - e_p))
//   f   = std(e_c) / std(e)                            per sample, unbiased (n - 1), as torch.std
//   out = e (phi f + 1 - phi)                          (phi = 0: out = e, no statistics at all)
//
// A work item is four consecutive elements of one sample; a wave is one 256-element chunk, a workgroup four chunks.  An item
// whose four elements lie inside the sample and whose addresses are all 16-byte aligned takes float4 loads and one float4 store,
// every other item up to four scalar ones: the values and the order of every operation are the same, so an element's bits do not
// depend on the path (file-wide contract(off) and explicit fmaf: the compiler fuses nothing on its own).
//
// fp32 roundings on an output's longest path: e_c - e_u, fmaf(w, ., e_u), e_c - e_p, fmaf(s, ., e) => e 4 (written as separate
// multiplies and adds it would be 6; the test's bound is stated for 6); phi > 0: the final multiply +1 => 5, besides the error
// of the factor itself.
//
// Statistics (phi > 0): each chunk's (mean, M2 = sum of squared deviations from ITS mean) of e_c and of e, two passes over the
// registers of one wave (xor butterflies: all 64 lanes end with the same bits); the chunks are merged in ascending order with
// Chan's update  d = mean_b - mean_a,  mean = mean_a + d n_b / n,  M2 = M2_a + M2_b + d^2 n_a n_b / n.
//   per_sample <= 1024: guidance_single_kernel, one workgroup per sample, the partials through LDS, e kept in registers;
//   larger:             guidance_stats_kernel writes one partial per chunk, [n_samples][chunks][4]; guidance_apply_kernel merges
//                       them (every thread the same loop) and recomputes e from its inputs.
// No atomics; a sample's bits depend on that sample alone, not on the run, the batch or its position in it.
// Every load of an item is issued before its store, so out may be e_c itself.
#include "../../include/adaface_hip.h"
#include "af_device.h"
#include "af_kernels.h"
#include <cmath>

#pragma clang fp contract(off)

namespace guid {

constexpr int IPT = 4;                    // elements of a work item
constexpr int CHUNK = AF_WAVE * IPT;      // elements of a wave: one statistics chunk
constexpr int WPB = 4;                    // waves (chunks) of a workgroup
constexpr int SINGLE_MAX = WPB * CHUNK;   // the largest sample guidance_single_kernel takes

struct Args {
  const float* ec;
  const float* eu;
  const float* ep;
  float* out;
  float* factor;        // [n_samples] or null
  float* part;          // chunked form: [n_samples][nchunk][4] = (mean, M2) of e_c, (mean, M2) of e
  long per_sample;
  int nchunk;           // ceil(per_sample / CHUNK)
  int nblk;             // workgroups per sample, ceil(nchunk / WPB)
  float w, s, phi, one_minus_phi;
};

struct Item {
  float ec[IPT], eu[IPT], ep[IPT];
  int n;                // elements of the item inside the sample, 0 .. 4
  bool wide;
};

template <bool CFG, bool PAG> __device__ __forceinline__ float combine(const Args& a, float ec, float eu, float ep) {
  float e = ec;
  if (CFG) e = fmaf(a.w, ec - eu, eu);
  if (PAG) e = fmaf(a.s, ec - ep, e);
  return e;
}

// the item at elements [i0, i0 + 4) of the sample that starts at element `base`; what lies beyond the sample reads as 0
template <bool CFG, bool PAG> __device__ __forceinline__ void load_item(const Args& a, long base, long i0, Item& it) {
  const long left = a.per_sample - i0;
  it.n = left >= IPT ? IPT : (left > 0 ? (int)left : 0);
  const long o = base + i0;
  uintptr_t bits = (uintptr_t)(a.ec + o) | (uintptr_t)(a.out + o);
  if (CFG) bits |= (uintptr_t)(a.eu + o);
  if (PAG) bits |= (uintptr_t)(a.ep + o);
  it.wide = it.n == IPT && (bits & 15) == 0;
#pragma unroll
  for (int k = 0; k < IPT; ++k) it.ec[k] = it.eu[k] = it.ep[k] = 0.f;
  if (it.wide) {
    const float4 c = *reinterpret_cast<const float4*>(a.ec + o);
    it.ec[0] = c.x; it.ec[1] = c.y; it.ec[2] = c.z; it.ec[3] = c.w;
    if (CFG) {
      const float4 u = *reinterpret_cast<const float4*>(a.eu + o);
      it.eu[0] = u.x; it.eu[1] = u.y; it.eu[2] = u.z; it.eu[3] = u.w;
    }
    if (PAG) {
      const float4 p = *reinterpret_cast<const float4*>(a.ep + o);
      it.ep[0] = p.x; it.ep[1] = p.y; it.ep[2] = p.z; it.ep[3] = p.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < IPT; ++k)
      if (k < it.n) {
        it.ec[k] = a.ec[o + k];
        if (CFG) it.eu[k] = a.eu[o + k];
        if (PAG) it.ep[k] = a.ep[o + k];
      }
  }
}

__device__ __forceinline__ void store_item(const Args& a, long base, long i0, const Item& it, const float (&v)[IPT]) {
  float* o = a.out + base + i0;
  if (it.wide) {
    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < IPT; ++k)
      if (k < it.n) o[k] = v[k];
  }
}

// (mean, M2) of the wave's chunk: cnt elements, lane-local sums in element order, then the butterflies.  Elements beyond the
// sample hold 0 and are left out of the second pass.  All 64 lanes call this and end with the same bits.
__device__ __forceinline__ float2 chunk_stats(const float (&v)[IPT], int n, float cnt) {
  const float mean = wave_sum(((v[0] + v[1]) + v[2]) + v[3]) / cnt;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < IPT; ++k)
    if (k < n) {
      const float d = v[k] - mean;
      q = fmaf(d, d, q);
    }
  return float2{mean, wave_sum(q)};
}

struct Stat { float mean, m2; };
// chunk b (nb elements) joins the na elements merged so far
__device__ __forceinline__ void merge(Stat& a, float na, float mb, float m2b, float nb) {
  const float n = na + nb;
  const float d = mb - a.mean;
  a.mean = fmaf(d, nb / n, a.mean);
  a.m2 = (a.m2 + m2b) + (d * d) * (na * nb / n);
}

// the sample's f = std(e_c) / std(e) from its chunk partials p[chunk][4], ascending
__device__ __forceinline__ float factor_of(const float* p, int nchunk, long per_sample) {
  Stat c{p[0], p[1]}, e{p[2], p[3]};
  float na = (float)(per_sample < CHUNK ? per_sample : CHUNK);
  for (int k = 1; k < nchunk; ++k) {
    const long left = per_sample - (long)k * CHUNK;
    const float nb = (float)(left < CHUNK ? left : CHUNK);
    merge(c, na, p[4 * k], p[4 * k + 1], nb);
    merge(e, na, p[4 * k + 2], p[4 * k + 3], nb);
    na += nb;
  }
  const float dof = (float)(per_sample - 1);
  return sqrtf(c.m2 / dof) / sqrtf(e.m2 / dof);
}

// phi = 0.  grid n_samples * nblk
template <bool CFG, bool PAG> __global__ __launch_bounds__(256) void guidance_combine_kernel(const Args a) {
  const long b = blockIdx.x / a.nblk;
  const int blk = blockIdx.x - (unsigned)(b * a.nblk);
  const long i0 = ((long)blk * WPB + threadIdx.x / AF_WAVE) * CHUNK + (threadIdx.x % AF_WAVE) * IPT;
  if (i0 >= a.per_sample) return;
  Item it;
  load_item<CFG, PAG>(a, b * a.per_sample, i0, it);
  float e[IPT];
#pragma unroll
  for (int k = 0; k < IPT; ++k) e[k] = combine<CFG, PAG>(a, it.ec[k], it.eu[k], it.ep[k]);
  store_item(a, b * a.per_sample, i0, it, e);
}

// phi > 0, per_sample <= SINGLE_MAX.  grid n_samples
template <bool CFG, bool PAG> __global__ __launch_bounds__(256) void guidance_single_kernel(const Args a) {
  __shared__ float part[WPB * 4];
  const long b = blockIdx.x;
  const int wave = threadIdx.x / AF_WAVE, lane = threadIdx.x % AF_WAVE;
  const long i0 = (long)wave * CHUNK + lane * IPT;
  Item it;
  load_item<CFG, PAG>(a, b * a.per_sample, i0, it);
  float e[IPT];
#pragma unroll
  for (int k = 0; k < IPT; ++k) e[k] = combine<CFG, PAG>(a, it.ec[k], it.eu[k], it.ep[k]);
  if (wave < a.nchunk) {   // (wave-uniform)
    const long left = a.per_sample - (long)wave * CHUNK;
    const float cnt = (float)(left < CHUNK ? left : CHUNK);
    const float2 sc = chunk_stats(it.ec, it.n, cnt), se = chunk_stats(e, it.n, cnt);
    if (lane == 0) { part[4 * wave] = sc.x; part[4 * wave + 1] = sc.y; part[4 * wave + 2] = se.x; part[4 * wave + 3] = se.y; }
  }
  __syncthreads();
  const float f = factor_of(part, a.nchunk, a.per_sample);
  if (threadIdx.x == 0 && a.factor) a.factor[b] = f;
  const float g = fmaf(a.phi, f, a.one_minus_phi);
#pragma unroll
  for (int k = 0; k < IPT; ++k) e[k] *= g;
  store_item(a, b * a.per_sample, i0, it, e);
}

// phi > 0, larger samples: one partial per chunk.  grid n_samples * nblk
template <bool CFG, bool PAG> __global__ __launch_bounds__(256) void guidance_stats_kernel(const Args a) {
  const long b = blockIdx.x / a.nblk;
  const int blk = blockIdx.x - (unsigned)(b * a.nblk);
  const int chunk = blk * WPB + threadIdx.x / AF_WAVE, lane = threadIdx.x % AF_WAVE;
  if (chunk >= a.nchunk) return;   // (wave-uniform; no barrier in this kernel)
  Item it;
  load_item<CFG, PAG>(a, b * a.per_sample, (long)chunk * CHUNK + lane * IPT, it);
  float e[IPT];
#pragma unroll
  for (int k = 0; k < IPT; ++k) e[k] = combine<CFG, PAG>(a, it.ec[k], it.eu[k], it.ep[k]);
  const long left = a.per_sample - (long)chunk * CHUNK;
  const float cnt = (float)(left < CHUNK ? left : CHUNK);
  const float2 sc = chunk_stats(it.ec, it.n, cnt), se = chunk_stats(e, it.n, cnt);
  if (lane == 0) *reinterpret_cast<float4*>(a.part + (b * a.nchunk + chunk) * 4) = make_float4(sc.x, sc.y, se.x, se.y);
}

// ... and the apply pass.  grid n_samples * nblk
template <bool CFG, bool PAG> __global__ __launch_bounds__(256) void guidance_apply_kernel(const Args a) {
  const long b = blockIdx.x / a.nblk;
  const int blk = blockIdx.x - (unsigned)(b * a.nblk);
  const float f = factor_of(a.part + b * a.nchunk * 4, a.nchunk, a.per_sample);
  if (blk == 0 && threadIdx.x == 0 && a.factor) a.factor[b] = f;
  const long i0 = ((long)blk * WPB + threadIdx.x / AF_WAVE) * CHUNK + (threadIdx.x % AF_WAVE) * IPT;
  if (i0 >= a.per_sample) return;
  const float g = fmaf(a.phi, f, a.one_minus_phi);
  Item it;
  load_item<CFG, PAG>(a, b * a.per_sample, i0, it);
  float e[IPT];
#pragma unroll
  for (int k = 0; k < IPT; ++k) e[k] = combine<CFG, PAG>(a, it.ec[k], it.eu[k], it.ep[k]) * g;
  store_item(a, b * a.per_sample, i0, it, e);
}

template <bool CFG, bool PAG> static int launch(const AfGuidancePlan& pl, const Args& a, long n_samples, hipStream_t s) {
  const dim3 grid((unsigned)(n_samples * a.nblk)), block(256);
  const double bytes = (double)n_samples * a.per_sample * 4.0 * (2 + (CFG ? 1 : 0) + (PAG ? 1 : 0));
  if (pl.kernel == AF_GDK_COMBINE) {
    AfProfScope prof(AF_K_GUIDANCE_APPLY, s, 0.0, bytes);
    hipLaunchKernelGGL((guidance_combine_kernel<CFG, PAG>), grid, block, 0, s, a);
  } else if (pl.kernel == AF_GDK_SINGLE) {
    AfProfScope prof(AF_K_GUIDANCE_APPLY, s, 0.0, bytes);
    hipLaunchKernelGGL((guidance_single_kernel<CFG, PAG>), dim3((unsigned)n_samples), block, 0, s, a);
  } else {
    {
      AfProfScope prof(AF_K_GUIDANCE_STATS, s, 0.0, bytes - (double)n_samples * a.per_sample * 4.0);
      hipLaunchKernelGGL((guidance_stats_kernel<CFG, PAG>), grid, block, 0, s, a);
      HIP_CHECK_RET(hipGetLastError());
    }
    AfProfScope prof(AF_K_GUIDANCE_APPLY, s, 0.0, bytes);
    hipLaunchKernelGGL((guidance_apply_kernel<CFG, PAG>), grid, block, 0, s, a);
  }
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

}  // namespace guid

// ---- host -----------------------------------------------------------------------------------------------------------------
int af_plan_guidance(long n_samples, long per_sample, bool rescale_on, AfGuidancePlan* pl) {
  *pl = AfGuidancePlan{AF_GDK_REFUSED, 0, 0, 0};
  if (n_samples < 1) { af_set_error_msg("guidance: %ld samples", n_samples); return -1; }
  if (per_sample < 2) { af_set_error_msg("guidance: per_sample %ld (the unbiased deviation needs >= 2 elements)", per_sample); return -1; }
  if (per_sample > (1L << 31)) { af_set_error_msg("guidance: per_sample %ld beyond 2^31", per_sample); return -1; }
  pl->nchunk = (per_sample + guid::CHUNK - 1) / guid::CHUNK;
  const long nblk = (pl->nchunk + guid::WPB - 1) / guid::WPB;
  if (nblk > 0x7fffffffL / n_samples) { af_set_error_msg("guidance: %ld x %ld is too large for one launch", n_samples, per_sample); return -1; }
  if (!rescale_on) { pl->kernel = AF_GDK_COMBINE; pl->launches = 1; }
  else if (per_sample <= guid::SINGLE_MAX) { pl->kernel = AF_GDK_SINGLE; pl->launches = 1; }
  else { pl->kernel = AF_GDK_CHUNKED; pl->launches = 2; pl->part_bytes = pl->nchunk * 4 * (long)sizeof(float); }
  return 0;
}

extern "C" {

int af_guidance_plan_query(int64_t n_samples, int64_t per_sample, int rescale_on, int64_t out[4]) {
  if (!out) { af_set_error_msg("af_guidance_plan_query: null output"); return AF_ERR_INVALID; }
  AfGuidancePlan pl;
  if (af_plan_guidance((long)n_samples, (long)per_sample, rescale_on != 0, &pl)) return AF_ERR_INVALID;
  out[0] = pl.kernel; out[1] = pl.launches; out[2] = pl.nchunk; out[3] = pl.part_bytes;
  return AF_OK;
}

int af_guidance(const float* eps_cond_dev, const float* eps_uncond_dev, const float* eps_pag_dev, int64_t n_samples,
                int64_t per_sample, float guidance, float pag_scale, float rescale, float* out_dev, float* factor_dev, void* stream) {
  if (!eps_cond_dev || !out_dev) { af_set_error_msg("af_guidance: null eps_cond or output"); return AF_ERR_INVALID; }
  if (!(rescale >= 0.f && rescale <= 1.f)) { af_set_error_msg("af_guidance: rescale %g outside [0, 1]", (double)rescale); return AF_ERR_INVALID; }
  AfGuidancePlan pl;
  if (af_plan_guidance((long)n_samples, (long)per_sample, rescale > 0.f, &pl)) return AF_ERR_INVALID;
  const int64_t n = n_samples * per_sample;
  auto overlaps = [](const float* p, int64_t np, const float* q, int64_t nq) {
    return p && q && (uintptr_t)p < (uintptr_t)(q + nq) && (uintptr_t)q < (uintptr_t)(p + np);
  };
  if ((out_dev != eps_cond_dev && overlaps(out_dev, n, eps_cond_dev, n)) || overlaps(out_dev, n, eps_uncond_dev, n) ||
      overlaps(out_dev, n, eps_pag_dev, n) || overlaps(factor_dev, n_samples, out_dev, n) ||
      overlaps(factor_dev, n_samples, eps_cond_dev, n) || overlaps(factor_dev, n_samples, eps_uncond_dev, n) ||
      overlaps(factor_dev, n_samples, eps_pag_dev, n)) {
    af_set_error_msg("af_guidance: the output may be eps_cond itself; any other overlap of output, factor and inputs is refused");
    return AF_ERR_INVALID;
  }
  if (pag_scale == 0.f) eps_pag_dev = nullptr;   // (e + 0 (e_c - e_p) is e: the same bits without the reads)
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  guid::Args a;
  a.ec = eps_cond_dev; a.eu = eps_uncond_dev; a.ep = eps_pag_dev;
  a.out = out_dev; a.factor = factor_dev; a.part = nullptr;
  a.per_sample = (long)per_sample;
  a.nchunk = (int)pl.nchunk;
  a.nblk = (int)((pl.nchunk + guid::WPB - 1) / guid::WPB);
  a.w = guidance; a.s = pag_scale; a.phi = rescale; a.one_minus_phi = 1.f - rescale;
  if (pl.kernel == AF_GDK_CHUNKED) {   // stream-ordered scratch for the chunk partials: no handle, no synchronisation
    void* p = nullptr;
    HIP_CHECK_RET(hipMallocAsync(&p, (size_t)n_samples * pl.part_bytes, s));
    a.part = reinterpret_cast<float*>(p);
  } else if (pl.kernel == AF_GDK_COMBINE && factor_dev) {
    af_set_error_msg("af_guidance: the factor is only computed with rescale > 0");
    return AF_ERR_INVALID;
  }
  int rc;
  if (a.eu && a.ep) rc = guid::launch<true, true>(pl, a, (long)n_samples, s);
  else if (a.eu) rc = guid::launch<true, false>(pl, a, (long)n_samples, s);
  else if (a.ep) rc = guid::launch<false, true>(pl, a, (long)n_samples, s);
  else rc = guid::launch<false, false>(pl, a, (long)n_samples, s);
  if (a.part) HIP_CHECK_RET(hipFreeAsync(a.part, s));
  return rc ? AF_ERR_HIP : AF_OK;
}

}  // extern "C"
