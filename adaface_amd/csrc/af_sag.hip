// adaface_amd — self-attention guidance: Hong, Lee, Jang, Kim, "Improving Sample Quality of Diffusion Models Using
// Self-Attention Guidance", ICCV 2023 (the arithmetic of diffusers' StableDiffusionSAGPipeline: sag_masking / gaussian_blur_2d,
// kernel size 9, threshold 1.0).  Two kernels and the one host function that states the Gaussian taps.  A translation unit of its
// own: the attention kernels of af_attention.hip never materialise probabilities and are not touched by it.
#include "../../include/adaface_hip.h"
#include "af_kernels.h"
#include <cmath>

std::atomic<long> g_af_sag_mass_launches{0};
std::atomic<long> g_af_sag_degrade_launches{0};

namespace sag {

// ---------------------------------------------------------------------------------------------------------------------------
// Attention mass per key of one self-attention site:
//   mass[b][j] = (1 / heads) sum_h sum_i softmax_j(q_bhi . k_bhj dh^-0.5),        fp32 [B][N]; its mean over j is 1.
// q and k are column views of the site's qkv activation: element (b, i, h dh + d) at p[b bs + i ld + h dh + d], storage type T,
// every product and sum in fp32.  No v, no attention output.
// Two launches, nothing atomic, every sum in a fixed order: a sample's result depends neither on its batch position nor on how
// the batch is split.  mass_kernel: ONE workgroup of four waves per (sample, head) writes that head's column sums
// part[b][h][N]; mass_heads_kernel adds the heads in ascending order and divides by their number.  A workgroup's walk is
// (query tile of TQ rows, chunk of DC head dims); per chunk K [N][DC] and Q [TQ][DC] are staged in LDS as fp32 (the next
// chunk's loads are in flight while this one is multiplied).  Wave w owns RPW query rows of the tile, lane l the keys l,
// l + 64, ..: a lane holds RPW x KJ score accumulators (k-ordered fmaf chains, d ascending), the softmax of a row is the exact
// max-subtracted form with the row maximum and the row sum reduced across the wave by xor butterflies (every lane gets the
// same bits), and p / sum goes into the lane's own column sums -- queries ascending within the wave.  The four waves' column
// sums are added in wave order at the end.
// N <= kMaxN = 256 (a 128 x 128 latent at the middle block, i.e. 1024 x 1024 pixels for SD-1.5): KJ = ceil(N / 64) <= 4 keys per
// lane, RPW KJ = 8 accumulators.  The scores go through the vector ALU, not the matrix cores: at N = 64, dh = 160, 8 heads a
// sample is 5.2 MFLOP, and an exact fp32 chain keeps the threshold mass > 1 comparable with a float64 restatement.
// ---------------------------------------------------------------------------------------------------------------------------
enum { kMaxN = 256, DC = 32, KLD = DC + 4, kThreads = 256 };   // KLD: a key row is 36 floats, so that 16 lanes' 16-byte reads of one
                                                                // column group fall on 16 different bank slots

template <typename T, bool VEC>
struct Pack {   // what one staging load brings: 16 bytes where the operands allow it, else one element
  static constexpr int EPC = VEC ? 16 / (int)sizeof(T) : 1;
  T e[EPC];
};

template <typename T, bool VEC>
__device__ __forceinline__ Pack<T, VEC> load_pack(const T* p, bool valid) {
  Pack<T, VEC> r;
  if constexpr (VEC) {
    uint4 u = make_uint4(0u, 0u, 0u, 0u);
    if (valid) u = *reinterpret_cast<const uint4*>(p);
    __builtin_memcpy(&r, &u, 16);
  } else {
    r.e[0] = valid ? p[0] : T(0.f);
  }
  return r;
}

template <typename T, bool VEC, int KJ>
__global__ __launch_bounds__(kThreads) void mass_kernel(const T* __restrict__ q, int ldq, long bsq, const T* __restrict__ k, int ldk,
                                                        long bsk, float* __restrict__ part, int N, int heads, int dh, float scale) {
  constexpr int RPW = 8 / KJ, TQ = 4 * RPW, KR = KJ * 64;
  constexpr int EPC = Pack<T, VEC>::EPC, VPR = DC / EPC;            // vectors per staged row
  constexpr int KPT = (KR * VPR + kThreads - 1) / kThreads, QPT = (TQ * VPR + kThreads - 1) / kThreads;
  __shared__ __attribute__((aligned(16))) float Ks[KR * KLD];
  __shared__ __attribute__((aligned(16))) float Qs[TQ * DC];
  __shared__ float Ws[4 * KR];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long b = blockIdx.y;
  const int h = blockIdx.x;
  const T* qb = q + b * bsq + (long)h * dh;
  const T* kb = k + b * bsk + (long)h * dh;
  const int ntiles = (N + TQ - 1) / TQ, nchunks = (dh + DC - 1) / DC;
  const int total = ntiles * nchunks;

  Pack<T, VEC> rk[KPT], rq[QPT];
  auto fetch = [&](int it) {
    const int c = it % nchunks, tile = it / nchunks;
    const int d0 = c * DC, q0 = tile * TQ;
#pragma unroll
    for (int u = 0; u < KPT; ++u) {
      const int idx = tid + u * kThreads, j = idx / VPR, d = d0 + (idx % VPR) * EPC;
      rk[u] = load_pack<T, VEC>(kb + (long)j * ldk + d, idx < KR * VPR && j < N && d < dh);
    }
#pragma unroll
    for (int u = 0; u < QPT; ++u) {
      const int idx = tid + u * kThreads, i = q0 + idx / VPR, d = d0 + (idx % VPR) * EPC;
      rq[u] = load_pack<T, VEC>(qb + (long)i * ldq + d, idx < TQ * VPR && i < N && d < dh);
    }
  };
  auto stage = [&]() {   // (rows >= N and head dims >= dh are zeros: they add nothing to a score)
#pragma unroll
    for (int u = 0; u < KPT; ++u) {
      const int idx = tid + u * kThreads;
      if (idx < KR * VPR) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) Ks[(idx / VPR) * KLD + (idx % VPR) * EPC + e] = to_f32<T>(rk[u].e[e]);
      }
    }
#pragma unroll
    for (int u = 0; u < QPT; ++u) {
      const int idx = tid + u * kThreads;
      if (idx < TQ * VPR) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) Qs[(idx / VPR) * DC + (idx % VPR) * EPC + e] = to_f32<T>(rq[u].e[e]);
      }
    }
  };

  float acc[RPW][KJ], col[KJ];
#pragma unroll
  for (int kj = 0; kj < KJ; ++kj) {
    col[kj] = 0.f;
#pragma unroll
    for (int r = 0; r < RPW; ++r) acc[r][kj] = 0.f;
  }
  fetch(0);
  for (int it = 0; it < total; ++it) {
    stage();
    __syncthreads();
    if (it + 1 < total) fetch(it + 1);
    const float* qrow = Qs + w * RPW * DC;
#pragma unroll
    for (int d = 0; d < DC; d += 4) {   // four head dims per 16-byte LDS read; every accumulator still takes them in ascending order
      float4 kv[KJ];
#pragma unroll
      for (int kj = 0; kj < KJ; ++kj) kv[kj] = *reinterpret_cast<const float4*>(&Ks[(lane + 64 * kj) * KLD + d]);
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        const float4 qv = *reinterpret_cast<const float4*>(&qrow[r * DC + d]);   // (one address per wave: a broadcast)
#pragma unroll
        for (int kj = 0; kj < KJ; ++kj) {
          float a = acc[r][kj];
          a = fmaf(qv.x, kv[kj].x, a);
          a = fmaf(qv.y, kv[kj].y, a);
          a = fmaf(qv.z, kv[kj].z, a);
          acc[r][kj] = fmaf(qv.w, kv[kj].w, a);
        }
      }
    }
    if (it % nchunks == nchunks - 1) {   // the tile's scores are complete: softmax over the keys, row by row
      const int q0 = (it / nchunks) * TQ + w * RPW;
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        float s[KJ], m = -INFINITY;
#pragma unroll
        for (int kj = 0; kj < KJ; ++kj) {
          s[kj] = lane + 64 * kj < N ? acc[r][kj] * scale : -INFINITY;
          m = fmaxf(m, s[kj]);
          acc[r][kj] = 0.f;
        }
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) m = fmaxf(m, __shfl_xor(m, sh, 64));
        float sum = 0.f;
#pragma unroll
        for (int kj = 0; kj < KJ; ++kj) {
          s[kj] = lane + 64 * kj < N ? expf(s[kj] - m) : 0.f;
          sum += s[kj];
        }
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) sum += __shfl_xor(sum, sh, 64);
        if (q0 + r < N) {   // (wave-uniform)
#pragma unroll
          for (int kj = 0; kj < KJ; ++kj) col[kj] += s[kj] / sum;
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int kj = 0; kj < KJ; ++kj) Ws[w * KR + lane + 64 * kj] = col[kj];
  __syncthreads();
  for (int j = tid; j < N; j += kThreads)
    part[(b * heads + h) * N + j] = ((Ws[j] + Ws[KR + j]) + Ws[2 * KR + j]) + Ws[3 * KR + j];
}

// mass[b][j] = (part[b][0][j] + part[b][1][j] + ..) / heads, the heads in ascending order
__global__ __launch_bounds__(kThreads) void mass_heads_kernel(const float* __restrict__ part, float* __restrict__ mass, long BN, int N,
                                                             int heads) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= BN) return;
  const long b = i / N, j = i - b * N;
  float s = 0.f;
  for (int h = 0; h < heads; ++h) s += part[(b * heads + h) * N + j];
  mass[i] = s / (float)heads;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The degraded input of the guide leg, fp32 [B][C][H][W], ONE launch:
//   x0    = (x - sigma e) / alpha
//   blur  = the separable 9-tap Gaussian of x0 per (sample, channel) plane, reflect padding of 4 (the edge pixel is not repeated)
//   d     = mass[b][(r / 8) (W / 8) + c / 8] > 1 ? blur : x0        (the mask cell of a pixel by index arithmetic)
//   x_deg = alpha d + sigma e
// A workgroup owns a band of BR rows of one plane: x0 of the band and a 4-row halo (reflected at the plane's edges) is computed
// into LDS, the horizontal pass runs LDS -> LDS over band + halo, the vertical pass reads it back; no mask, x0, blur or padded
// tensor reaches memory.  Every product-sum is an explicit fmaf.  fp32 roundings on the output's longest path, counted as if
// nothing were fused:
//   x0      mul, sub, IEEE division               3
//   h pass  w_0 v, then eight additions          +9  => 12     (the other eight products are rounded once each, off the path)
//   v pass  the same                             +9  => 21
//   x_deg   alpha d, + sigma e                   +2  => 23     (mask off: x0 straight to the last line, 3 + 2 = 5)
// Element loads and stores (consecutive lanes, consecutive columns): any 4-byte alignment.  W <= kMaxW so that two band images
// fit the default LDS limit.
// ---------------------------------------------------------------------------------------------------------------------------
enum { BR = 16, HALO = 4, kMaxW = 256 };

struct DegradeArgs {
  const float* x;
  const float* e;
  const float* mass;
  float* out;
  int C, H, W;
  float alpha, sigma;
  float w[9];
};

__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

__global__ __launch_bounds__(kThreads) void degrade_kernel(const DegradeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sag_lds[];
  const int H = a.H, W = a.W, tid = threadIdx.x;
  const int r0 = blockIdx.x * BR, rows = min(BR, H - r0), srows = rows + 2 * HALO;
  const long plane = blockIdx.y;
  const long base = plane * H * W;
  float* X0 = sag_lds;                       // [srows][W]: x0 of rows r0 - 4 .. r0 + rows + 3, reflected
  float* Hb = sag_lds + (BR + 2 * HALO) * W;   // [srows][W]: the horizontal pass of the same rows
  for (int idx = tid; idx < srows * W; idx += kThreads) {
    const int lr = idx / W, c = idx - lr * W;
    const long g = base + (long)reflect(r0 + lr - HALO, H) * W + c;
    X0[idx] = fmaf(-a.sigma, a.e[g], a.x[g]) / a.alpha;
  }
  __syncthreads();
  for (int idx = tid; idx < srows * W; idx += kThreads) {
    const int lr = idx / W, c = idx - lr * W;
    const float* row = X0 + lr * W;
    float s = a.w[0] * row[reflect(c - HALO, W)];
#pragma unroll
    for (int t = 1; t < 9; ++t) s = fmaf(a.w[t], row[reflect(c + t - HALO, W)], s);
    Hb[idx] = s;
  }
  __syncthreads();
  const int Wc = W >> 3;
  const float* mrow = a.mass + (plane / a.C) * (long)(H >> 3) * Wc;
  for (int idx = tid; idx < rows * W; idx += kThreads) {
    const int r = idx / W, c = idx - r * W;
    float s = a.w[0] * Hb[idx];
#pragma unroll
    for (int t = 1; t < 9; ++t) s = fmaf(a.w[t], Hb[idx + t * W], s);
    const bool on = mrow[((r0 + r) >> 3) * Wc + (c >> 3)] > 1.0f;
    const float d = on ? s : X0[idx + HALO * W];
    const long g = base + (long)(r0 + r) * W + c;
    a.out[g] = fmaf(a.alpha, d, a.sigma * a.e[g]);
  }
}

}  // namespace sag

template <typename T>
int af_launch_sag_mass(const void* q, int ldq, long bsq, const void* k, int ldk, long bsk, float* mass, float* part, int B, int N,
                       int heads, int dh, hipStream_t s) {
  using namespace sag;
  if (!q || !k || !mass || !part) { af_set_error_msg("sag mass: null operand"); return -1; }
  if (B < 0 || N <= 0 || heads <= 0 || dh <= 0) { af_set_error_msg("sag mass: bad shape B=%d N=%d heads=%d dh=%d", B, N, heads, dh); return -1; }
  if (N > kMaxN) { af_set_error_msg("sag mass: N = %d keys exceed the kernel's %d (a 128 x 128 latent at the middle block)", N, (int)kMaxN); return -1; }
  if ((long)heads * dh > ldq || (long)heads * dh > ldk || bsq < 0 || bsk < 0) {
    af_set_error_msg("sag mass: row strides %d / %d below heads * dh = %ld", ldq, ldk, (long)heads * dh);
    return -1;
  }
  if (B == 0) return 0;
  if (B > 65535 || heads > 65535) { af_set_error_msg("sag mass: B = %d / heads = %d are too many for one launch", B, heads); return -1; }
  constexpr int EPC = 16 / (int)sizeof(T);
  auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool vec = al(q) && al(k) && ldq % EPC == 0 && ldk % EPC == 0 && bsq % EPC == 0 && bsk % EPC == 0 && dh % EPC == 0;
  const float scale = (float)(1.0 / std::sqrt((double)dh));
  const dim3 grid((unsigned)heads, (unsigned)B), block(kThreads);
  const T* qp = reinterpret_cast<const T*>(q);
  const T* kp = reinterpret_cast<const T*>(k);
#define AF_SAG_MASS(V, KJ) hipLaunchKernelGGL((mass_kernel<T, V, KJ>), grid, block, 0, s, qp, ldq, bsq, kp, ldk, bsk, part, N, heads, dh, scale)
  if (vec) { if (N <= 64) AF_SAG_MASS(true, 1); else if (N <= 128) AF_SAG_MASS(true, 2); else AF_SAG_MASS(true, 4); }
  else { if (N <= 64) AF_SAG_MASS(false, 1); else if (N <= 128) AF_SAG_MASS(false, 2); else AF_SAG_MASS(false, 4); }
#undef AF_SAG_MASS
  HIP_CHECK_RET(hipGetLastError());
  const long BN = (long)B * N;
  hipLaunchKernelGGL(mass_heads_kernel, dim3((unsigned)((BN + kThreads - 1) / kThreads)), block, 0, s, part, mass, BN, N, heads);
  HIP_CHECK_RET(hipGetLastError());
  g_af_sag_mass_launches.fetch_add(1, std::memory_order_relaxed);
  return 0;
}

#define AF_SAG_INST(T) \
  template int af_launch_sag_mass<T>(const void*, int, long, const void*, int, long, float*, float*, int, int, int, int, hipStream_t);
AF_SAG_INST(bf16)
AF_SAG_INST(f16)
AF_SAG_INST(float)

extern "C" {

int64_t af_sag_mass_launches(void) { return (int64_t)g_af_sag_mass_launches.load(std::memory_order_relaxed); }
int64_t af_sag_degrade_launches(void) { return (int64_t)g_af_sag_degrade_launches.load(std::memory_order_relaxed); }

int af_sag_taps(double sigma, double out[9]) {
  // The only place of the product that states the Gaussian: w_i = exp(-0.5 ((i - 4) / sigma)^2) / sum, nine taps.
  if (!out) { af_set_error_msg("af_sag_taps: null output"); return AF_ERR_INVALID; }
  if (!std::isfinite(sigma) || !(sigma > 0.0)) { af_set_error_msg("af_sag_taps: blur sigma %g is not a positive number", sigma); return AF_ERR_INVALID; }
  double sum = 0.0;
  for (int i = 0; i < 9; ++i) {
    const double z = (double)(i - 4) / sigma;
    out[i] = std::exp(-0.5 * z * z);
    sum += out[i];
  }
  for (int i = 0; i < 9; ++i) out[i] /= sum;
  return AF_OK;
}

int af_sag_degrade(const float* x_dev, const float* eps_dev, const float* mass_dev, float* out_dev, int B, int C, int H, int W,
                   float alpha, float sigma, double blur_sigma, void* stream) {
  using namespace sag;
  if (!x_dev || !eps_dev || !mass_dev || !out_dev) { af_set_error_msg("af_sag_degrade: null argument"); return AF_ERR_INVALID; }
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || H % 8 || W % 8) {
    af_set_error_msg("af_sag_degrade: bad shape B=%d C=%d H=%d W=%d (H and W positive multiples of 8)", B, C, H, W);
    return AF_ERR_INVALID;
  }
  if (W > kMaxW) { af_set_error_msg("af_sag_degrade: W = %d exceeds the kernel's %d columns", W, (int)kMaxW); return AF_ERR_INVALID; }
  const long planes = (long)B * C, n = planes * H * W;
  if (planes > 65535 || n > 0x7fffffffL) { af_set_error_msg("af_sag_degrade: %ld planes / %ld elements are too many for one launch", planes, n); return AF_ERR_INVALID; }
  if (!(alpha > 0.f) || !std::isfinite(alpha) || !std::isfinite(sigma)) { af_set_error_msg("af_sag_degrade: alpha %g is not positive (sigma %g)", (double)alpha, (double)sigma); return AF_ERR_INVALID; }
  double taps[9];
  if (af_sag_taps(blur_sigma, taps) != AF_OK) return AF_ERR_INVALID;
  const long nm = (long)B * (H / 8) * (W / 8);
  auto overlaps = [](const float* p, long np, const float* q, long nq) {
    return (uintptr_t)p < (uintptr_t)(q + nq) && (uintptr_t)q < (uintptr_t)(p + np);
  };
  if (overlaps(out_dev, n, x_dev, n) || overlaps(out_dev, n, eps_dev, n) || overlaps(out_dev, n, mass_dev, nm)) {
    af_set_error_msg("af_sag_degrade: the output must not alias x, eps or the mass (a band reads its neighbours' rows)");
    return AF_ERR_INVALID;
  }
  DegradeArgs a{x_dev, eps_dev, mass_dev, out_dev, C, H, W, alpha, sigma, {}};
  for (int i = 0; i < 9; ++i) a.w[i] = (float)taps[i];   // rounded to fp32 once, here
  const dim3 grid((unsigned)((H + BR - 1) / BR), (unsigned)planes), block(kThreads);
  const size_t lds = (size_t)2 * (BR + 2 * HALO) * W * sizeof(float);
  hipLaunchKernelGGL(degrade_kernel, grid, block, lds, reinterpret_cast<hipStream_t>(stream), a);
  HIP_CHECK_RET(hipGetLastError());
  g_af_sag_degrade_launches.fetch_add(1, std::memory_order_relaxed);
  return AF_OK;
}

}  // extern "C"
