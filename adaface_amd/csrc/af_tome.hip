// adaface_amd — token merging (ToMe) in front of the U-Net's self-attention: Bolya & Hoffman, "Token Merging for
// Fast Stable Diffusion" (CVPR-W 2023), the tomesd package with sx = sy = 2, use_rand = False, merge_attn only.
//
// A map of H x W tokens (both even, raster order i = y W + x) is split into dst tokens (y and x even; ordinal
// d = (y / 2) (W / 2) + x / 2, Nd = N / 4 of them) and src tokens (the others, ordinal s in raster order, Ns = N - Nd).
//   tome_rnorm_kernel      rn_i = (sum t_i^2)^-1/2 of every token, fp32, 0 for a zero row             (normalize only)
//   tome_match_*_kernel    node_max[s] = max_d t_s . t_d rn_s rn_d, node_idx[s] = the lowest d attaining it; the score matrix
//                          is never stored.  bf16: src rows resident as MFMA fragments, dst tiles through LDS.  Any other
//                          storage type or width: plain FMA.
//   tome_rank_kernel       merged[s] = fewer than r pairs (node_max, s') order before (node_max[s], s): larger value first,
//                          ties to the lower ordinal.  Counting, no sort, no atomics.
//   tome_map_kernel        prefix sum over the unmerged src tokens -> map[i] in [0, N'), N' = N - r: rows 0 .. Nd-1 are the dst
//                          tokens, rows Nd .. N'-1 the unmerged src tokens in raster order, a merged src token maps to node_idx
//   tome_merge_kernel      row j of the merged sequence = mean over {i : map[i] = j} of LayerNorm(t_i), fp32 values summed in
//                          ascending i, rounded once.  A gather: every row scans the sample's map, nothing is scattered.
//   tome_unmerge_add_kernel  t1_i = t_i + o[map[i]] in fp32, rounded once; optionally the LayerNorm row sums of t1 in the layout
//                          of ConvGemmParams::ln_stats_out.
// Everything is deterministic: fixed summation orders, no atomics.
#include "af_kernels.h"

#include <type_traits>

namespace tome {

// token index of src ordinal s / dst ordinal d on a map W wide (W even)
__device__ __forceinline__ int src_token(int s, int W) {
  const int per = W + (W >> 1);   // src tokens of a row pair: W / 2 on the even row, W on the odd one
  const int p = s / per, rem = s - p * per;
  return rem < (W >> 1) ? (2 * p) * W + 2 * rem + 1 : (2 * p + 1) * W + (rem - (W >> 1));
}
__device__ __forceinline__ int dst_token(int d, int W) {
  const int hw = W >> 1;
  const int dy = d / hw;
  return 2 * dy * W + 2 * (d - dy * hw);
}
__device__ __forceinline__ bool is_dst(int i, int W) {
  const int y = i / W, x = i - y * W;
  return ((y | x) & 1) == 0;
}

constexpr int LN_MAXV = 5;   // as layernorm_kernel: C * sizeof(T) / 16 <= 64 * 5 vectors

// The row arithmetic of layernorm_kernel (af_norm.hip), statement for statement, on a wave that holds row `xr` (lane l: vectors
// l, l + 64, ...): the fp32 values that kernel rounds and stores.  gamma == null: no LayerNorm, the stored values.
// Where hipcc is free to contract a multiply and an add, the form that kernel's code object has is spelled out: contraction is
// off in this function and the one fma is written as such (inside this kernel's larger body the compiler had fused part of a
// row's sum of squares); tests/test_tome_gpu.py holds the two to the same bits, rows with one member against af_op_layernorm.
// MAXV: vectors a lane holds at most, ceil(NV / 64) <= LN_MAXV (that kernel's fifth-vector guards, for a narrower row, skip what
// is not unrolled here: the same additions in the same order).
template <typename T, int MAXV>
__device__ __forceinline__ void ln_row_wave(const T* __restrict__ xr, int NV, int Cn, int lane, const float* __restrict__ gamma,
                                            const float* __restrict__ beta, float eps, float (&ff)[MAXV][16 / sizeof(T)]) {
#pragma clang fp contract(off)
  constexpr int EPC = 16 / sizeof(T);
  Vec16<T> v[MAXV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int vi = lane + 64 * i;
    if (vi < NV) {
      v[i].u = *reinterpret_cast<const uint4*>(xr + vi * EPC);
#pragma unroll
      for (int e = 0; e < EPC; ++e) s += to_f32<T>(v[i].e[e]);
    }
  }
  if (!gamma) {
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
#pragma unroll
      for (int e = 0; e < EPC; ++e) ff[i][e] = (lane + 64 * i < NV) ? to_f32<T>(v[i].e[e]) : 0.f;
    return;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const float mean = s / (float)Cn;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int vi = lane + 64 * i;
    if (vi < NV) {
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        const float d = to_f32<T>(v[i].e[e]) - mean;
        q += d * d;   // (a separate multiply and add, as that kernel's code has them: contraction is off in this function)
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  const float rstd = rsqrtf(q / (float)Cn + eps);
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int vi = lane + 64 * i;
#pragma unroll
    for (int e = 0; e < EPC; ++e) ff[i][e] = 0.f;
    if (vi < NV) {
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        const int c = vi * EPC + e;
        ff[i][e] = __builtin_fmaf((to_f32<T>(v[i].e[e]) - mean) * rstd, gamma[c], beta[c]);   // (... and its one fma)
      }
    }
  }
}

// ---- reciprocal norms: one wave per token ---------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void tome_rnorm_kernel(const T* __restrict__ x, int ldx, long rows, int Cn, float* __restrict__ rn) {
  constexpr int EPC = 16 / sizeof(T);
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int NV = Cn / EPC;
  float s = 0.f;
  for (int vi = lane; vi < NV; vi += 64) {
    Vec16<T> v;
    v.u = *reinterpret_cast<const uint4*>(x + row * ldx + vi * EPC);
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const float f = to_f32<T>(v.e[e]);
      s += f * f;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) rn[row] = s > 0.f ? 1.0f / sqrtf(s) : 0.f;
}

// ---- match, bf16 on the MFMA ----------------------------------------------------------------------------------------------
// A workgroup of four waves owns 128 src tokens of one sample, a wave 32 of them: their rows stay in registers as the B
// operand fragments of v_mfma_f32_32x32x16_bf16 (NK = C / 16 fragments of 16 bytes per lane).  The dst tokens pass through LDS
// in tiles of 32 rows (the A operand), two buffers, one barrier per tile: tile t + 1 is fetched into registers before the
// MFMAs of tile t and written to the other buffer after them.  In this (swapped) form the accumulator column of a lane is ONE
// src token (lane & 31) and its 16 registers are 16 dst tokens in ascending order, so the running (max, argmax) is lane-local;
// the two lane halves hold the other 16 dst rows of the same src token and are combined once, at the end, on (value, index).
// LDS rows are C * 2 + 16 bytes apart: the 16 lanes of a ds_read_b128 group then fall on 16 different 16-byte slots of the
// 256-byte bank row (row stride mod 256 bytes = 16 * odd or 16, for every C that is a multiple of 64).
template <int NK>
__global__ __launch_bounds__(256) void tome_match_mfma_kernel(const bf16* __restrict__ x, int ldx, int W, int Nd, int Ns,
                                                               const float* __restrict__ rn, int* __restrict__ node_idx,
                                                               float* __restrict__ node_max) {
  constexpr int C = NK * 16;
  constexpr int ROWB = C * 2 + 16;               // bytes between LDS rows
  constexpr int VPR = NK * 2;                    // 16-byte vectors per row
  constexpr int VPT = 32 * VPR / 256;            // vectors a thread stages per tile
  static_assert(NK % 4 == 0, "a tile is staged in whole rounds of the workgroup");
  extern __shared__ __attribute__((aligned(16))) char s_match[];   // tiles [2][32 * ROWB] | rn of their rows [2][32]
  auto tile_of = [&](int buf) { return s_match + buf * (32 * ROWB); };
  auto rn_of = [&](int buf) { return reinterpret_cast<float*>(s_match + 2 * 32 * ROWB) + buf * 32; };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
  const int b = blockIdx.y;
  const long N = (long)Nd + Ns;
  const bf16* xb = x + (long)b * N * ldx;
  const float* rnb = rn ? rn + (long)b * N : nullptr;

  const int s_own = blockIdx.x * 128 + wave * 32 + l31;
  const int s_ld = s_own < Ns ? s_own : Ns - 1;   // (lanes past the last src token compute a copy of it and store nothing)
  const int i_src = src_token(s_ld, W);
  uint4 sf[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) sf[k] = *reinterpret_cast<const uint4*>(xb + (long)i_src * ldx + 16 * k + 8 * half);
  const float rn_s = rnb ? rnb[i_src] : 1.0f;

  const int ntile = (Nd + 31) / 32;
  uint4 st[VPT];
  float st_rn = 0.f;
  auto fetch = [&](int t) {
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
      const int idx = tid + 256 * u, r = idx / VPR, vv = idx - r * VPR;
      const int d = t * 32 + r;
      st[u] = d < Nd ? *reinterpret_cast<const uint4*>(xb + (long)dst_token(d, W) * ldx + vv * 8) : uint4{0u, 0u, 0u, 0u};
    }
    if (tid < 32) {
      const int d = t * 32 + tid;
      st_rn = (rnb && d < Nd) ? rnb[dst_token(d, W)] : 1.0f;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
      const int idx = tid + 256 * u, r = idx / VPR, vv = idx - r * VPR;
      *reinterpret_cast<uint4*>(tile_of(buf) + r * ROWB + vv * 16) = st[u];
    }
    if (tid < 32) rn_of(buf)[tid] = st_rn;
  };
  fetch(0);
  stash(0);
  __syncthreads();

  float best = -__builtin_inff();
  int bidx = 0;
  for (int t = 0; t < ntile; ++t) {
    const int buf = t & 1;
    if (t + 1 < ntile) fetch(t + 1);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const char* arow = tile_of(buf) + l31 * ROWB + 16 * half;
    const float* rn_t = rn_of(buf);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const uint4 a = *reinterpret_cast<const uint4*>(arow + 32 * k);
      Mma<bf16>::step(a, sf[k], acc);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rr = acc_row(r, half);
      const int d = t * 32 + rr;
      float v = acc[r];
      if (rnb) v = v * rn_s * rn_t[rr];
      if (d < Nd && v > best) { best = v; bidx = d; }   // (d ascends with r and t: strict > keeps the lowest index)
    }
    if (t + 1 < ntile) stash(buf ^ 1);
    __syncthreads();
  }
  const float ob = __shfl_xor(best, 32, 64);
  const int oi = __shfl_xor(bidx, 32, 64);
  if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
  if (half == 0 && s_own < Ns) {
    node_idx[(long)b * Ns + s_own] = bidx;
    node_max[(long)b * Ns + s_own] = best;
  }
}

// ---- match, any storage type and width: plain FMA -------------------------------------------------------------------------
// 64 src tokens per workgroup; thread (ts = tid & 63, g = tid >> 6) accumulates src ts against 16 dst tokens of each 64-row dst
// tile, K in chunks of 32 through LDS (fp32, rows 33 floats apart).
template <typename T>
__global__ __launch_bounds__(256) void tome_match_plain_kernel(const T* __restrict__ x, int ldx, int W, int Nd, int Ns, int Cn,
                                                                const float* __restrict__ rn, int* __restrict__ node_idx,
                                                                float* __restrict__ node_max) {
  constexpr int KC = 32;
  __shared__ float s_src[64][KC + 1];
  __shared__ float s_dst[64][KC + 1];
  __shared__ float s_bv[4][64];
  __shared__ int s_bi[4][64];
  const int tid = threadIdx.x, ts = tid & 63, g = tid >> 6;
  const int b = blockIdx.y;
  const long N = (long)Nd + Ns;
  const T* xb = x + (long)b * N * ldx;
  const float* rnb = rn ? rn + (long)b * N : nullptr;
  const int s0 = blockIdx.x * 64;
  const int s_own = s0 + ts;
  const float rn_s = (rnb && s_own < Ns) ? rnb[src_token(s_own, W)] : 1.0f;
  float best = -__builtin_inff();
  int bidx = 0;
  for (int d0 = 0; d0 < Nd; d0 += 64) {
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    for (int k0 = 0; k0 < Cn; k0 += KC) {
      __syncthreads();
      for (int idx = tid; idx < 64 * KC; idx += 256) {
        const int r = idx / KC, k = idx - r * KC;
        const int s = s0 + r, d = d0 + r;
        const bool kin = k0 + k < Cn;
        s_src[r][k] = (s < Ns && kin) ? to_f32<T>(xb[(long)src_token(s, W) * ldx + k0 + k]) : 0.f;
        s_dst[r][k] = (d < Nd && kin) ? to_f32<T>(xb[(long)dst_token(d, W) * ldx + k0 + k]) : 0.f;
      }
      __syncthreads();
#pragma unroll 4
      for (int k = 0; k < KC; ++k) {
        const float a = s_src[ts][k];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = fmaf(a, s_dst[g * 16 + j][k], acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int d = d0 + g * 16 + j;
      float v = acc[j];
      if (rnb && d < Nd) v = v * rn_s * rnb[dst_token(d, W)];
      if (d < Nd && v > best) { best = v; bidx = d; }
    }
  }
  s_bv[g][ts] = best;
  s_bi[g][ts] = bidx;
  __syncthreads();
  if (g == 0 && s_own < Ns) {
#pragma unroll
    for (int o = 1; o < 4; ++o) {
      const float ob = s_bv[o][ts];
      const int oi = s_bi[o][ts];
      if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    node_idx[(long)b * Ns + s_own] = bidx;
    node_max[(long)b * Ns + s_own] = best;
  }
}

// ---- select ---------------------------------------------------------------------------------------------------------------
// One thread per src token; the sample's node_max values pass through LDS 1024 at a time (-inf behind the last one, which orders
// before nothing) and are read sixteen per step as broadcast 16-byte reads.  (Read one by one the loop ran at the LDS latency,
// 81 us per launch at Ns = 3072; with wave-uniform global addresses -- scalar loads -- at the scalar cache's, 141 us.)
__global__ __launch_bounds__(256) void tome_rank_kernel(const float* __restrict__ node_max, int Ns, int r, int* __restrict__ merged) {
  __shared__ __attribute__((aligned(16))) float s_v[1024];
  const int b = blockIdx.y;
  const float* nm = node_max + (long)b * Ns;
  const int s = blockIdx.x * 256 + threadIdx.x;
  const float v = s < Ns ? nm[s] : 0.f;
  int before = 0;
  for (int c0 = 0; c0 < Ns; c0 += 1024) {
    __syncthreads();
    for (int j = threadIdx.x; j < 1024; j += 256) s_v[j] = c0 + j < Ns ? nm[c0 + j] : -__builtin_inff();
    __syncthreads();
    for (int j = 0; j < 1024; j += 16) {
      float u[16];
#pragma unroll
      for (int k = 0; k < 4; ++k) *reinterpret_cast<float4*>(u + 4 * k) = *reinterpret_cast<const float4*>(s_v + j + 4 * k);
#pragma unroll
      for (int k = 0; k < 16; ++k) before += (u[k] > v ? 1 : 0) + ((u[k] == v && c0 + j + k < s) ? 1 : 0);
    }
  }
  if (s < Ns) merged[(long)b * Ns + s] = before < r ? 1 : 0;
}

// one workgroup per sample: thread t owns the src ordinals [t * per, (t + 1) * per)
__global__ __launch_bounds__(256) void tome_map_kernel(const int* __restrict__ merged, const int* __restrict__ node_idx, int W,
                                                        int Nd, int Ns, int* __restrict__ map) {
  __shared__ int s_cnt[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int* mg = merged + (long)b * Ns;
  const int* ni = node_idx + (long)b * Ns;
  int* mp = map + (long)b * ((long)Nd + Ns);
  const int per = (Ns + 255) / 256;
  const int lo = tid * per < Ns ? tid * per : Ns, hi = lo + per < Ns ? lo + per : Ns;
  int cnt = 0;
  for (int s = lo; s < hi; ++s) cnt += mg[s] ? 0 : 1;
  s_cnt[tid] = cnt;
  __syncthreads();
  int row = Nd;
  for (int t = 0; t < tid; ++t) row += s_cnt[t];   // (256 LDS broadcast reads: the exclusive prefix in a fixed order)
  for (int s = lo; s < hi; ++s) {
    const int i = src_token(s, W);
    if (mg[s]) {
      const int d = ni[s];
      mp[i] = d < 0 ? 0 : (d >= Nd ? Nd - 1 : d);
    } else {
      mp[i] = row++;
    }
  }
  for (int d = tid; d < Nd; d += 256) mp[dst_token(d, W)] = d;
}

// ---- LayerNorm + merge ----------------------------------------------------------------------------------------------------
// A workgroup owns MERGE_ROWS consecutive rows of one sample's merged sequence, a wave a quarter of them.  The sample's map sits
// in LDS (dynamic: N ints, filled with -1 up to a multiple of 256); for each of its rows a wave scans it 256 tokens at a time
// (lane l: tokens 4 l .. 4 l + 3 of the step, one ds_read_b128) and adds the members in ascending token order.  MAXV vectors per
// lane keep the kernel at the registers its row width needs: the waves in flight hide the members' load latency.
constexpr int MERGE_ROWS = 16;
template <typename T, int MAXV>
__global__ __launch_bounds__(256) void tome_merge_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, const int* __restrict__ map,
                                                          int N, int Np, int Cn, T* __restrict__ y, int ldy) {
  constexpr int EPC = 16 / sizeof(T);
  extern __shared__ __attribute__((aligned(16))) int s_map[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const int* mp = map + (long)b * N;
  const int Npad = (N + 255) & ~255;
  for (int i = tid; i < Npad; i += 256) s_map[i] = i < N ? mp[i] : -1;
  __syncthreads();
  const T* xb = x + (long)b * N * ldx;
  T* yb = y + (long)b * Np * ldy;
  const int NV = Cn / EPC;
  for (int jj = 0; jj < MERGE_ROWS / 4; ++jj) {
    const int j = blockIdx.x * MERGE_ROWS + wave * (MERGE_ROWS / 4) + jj;   // (wave-uniform)
    if (j >= Np) break;
    float acc[MAXV][EPC];
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
#pragma unroll
      for (int e = 0; e < EPC; ++e) acc[i][e] = 0.f;
    int cnt = 0;
    for (int i0 = 0; i0 < Npad; i0 += 256) {
      const int4 mv = *reinterpret_cast<const int4*>(s_map + i0 + 4 * lane);
      const unsigned long long m0 = __ballot(mv.x == j), m1 = __ballot(mv.y == j), m2 = __ballot(mv.z == j), m3 = __ballot(mv.w == j);
      unsigned long long any = m0 | m1 | m2 | m3;
      while (any) {   // (lanes ascending, a lane's four tokens ascending: ascending token order)
        const int bit = __builtin_ctzll(any);
        any &= any - 1;
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
          const unsigned long long me = e4 == 0 ? m0 : e4 == 1 ? m1 : e4 == 2 ? m2 : m3;
          if (!((me >> bit) & 1ull)) continue;
          float ff[MAXV][EPC];
          ln_row_wave<T, MAXV>(xb + (long)(i0 + 4 * bit + e4) * ldx, NV, Cn, lane, gamma, beta, eps, ff);
#pragma unroll
          for (int v = 0; v < MAXV; ++v)
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[v][e] += ff[v][e];
          ++cnt;
        }
      }
    }
    const float div = (float)(cnt > 0 ? cnt : 1);
#pragma unroll
    for (int v = 0; v < MAXV; ++v) {
      const int vi = lane + 64 * v;
      if (vi < NV) {
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < EPC; ++e) o.e[e] = from_f32<T>(acc[v][e] / div);
        *reinterpret_cast<uint4*>(yb + (long)j * ldy + vi * EPC) = o.u;
      }
    }
  }
}

// ---- unmerge + residual: one wave per token -------------------------------------------------------------------------------
// stats != null: the sum and the sum of squares of the ROUNDED values of every row, as a LayerNorm producer GEMM leaves them
// (ConvGemmParams::ln_stats_out, [parts][rows][2]): the whole row in part 0, zeros in the other parts -- the consumers add the
// parts up.
template <typename T>
__global__ __launch_bounds__(256) void tome_unmerge_add_kernel(const T* __restrict__ o, int ldo, const T* __restrict__ res, int ldr,
                                                                const int* __restrict__ map, int N, int Np, long rows, int Cn,
                                                                T* __restrict__ y, int ldy, float* __restrict__ stats, int parts) {
  constexpr int EPC = 16 / sizeof(T);
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long b = row / N;
  int j = map[row];
  j = j < 0 ? 0 : (j >= Np ? Np - 1 : j);
  const T* orow = o + (b * Np + j) * ldo;
  const int NV = Cn / EPC;
  float s1 = 0.f, s2 = 0.f;
  for (int vi = lane; vi < NV; vi += 64) {
    Vec16<T> a, r, out;
    a.u = *reinterpret_cast<const uint4*>(orow + vi * EPC);
    r.u = *reinterpret_cast<const uint4*>(res + row * ldr + vi * EPC);
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      out.e[e] = from_f32<T>(to_f32<T>(r.e[e]) + to_f32<T>(a.e[e]));
      const float f = to_f32<T>(out.e[e]);
      s1 += f;
      s2 += f * f;
    }
    *reinterpret_cast<uint4*>(y + row * ldy + vi * EPC) = out.u;
  }
  if (stats) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
      s1 += __shfl_xor(s1, sh, 64);
      s2 += __shfl_xor(s2, sh, 64);
    }
    for (int p = lane; p < parts; p += 64) {
      float* d = stats + ((long)p * rows + row) * 2;
      d[0] = p == 0 ? s1 : 0.f;
      d[1] = p == 0 ? s2 : 0.f;
    }
  }
}

}  // namespace tome

// ---- host -----------------------------------------------------------------------------------------------------------------
int af_tome_plan(int H, int W, double ratio, AfTomePlan* pl) {
  if (H <= 0 || W <= 0 || (H & 1) || (W & 1)) {
    af_set_error_msg("token merging: the map must have even, positive sides, got %d x %d", H, W);
    return -1;
  }
  if (!(ratio >= 0.0 && ratio <= 0.75)) {
    af_set_error_msg("token merging: ratio %g outside [0, 0.75]", ratio);
    return -1;
  }
  const long N = (long)H * W;
  pl->Nd = N / 4;
  pl->Ns = N - pl->Nd;
  const long want = (long)((double)N * ratio);   // (truncation, as Python's int())
  pl->r = want < pl->Ns ? want : pl->Ns;
  pl->Np = N - pl->r;
  return 0;
}

size_t af_tome_match_ws_bytes(int B, int H, int W) {
  const size_t N = (size_t)H * W;
  return (size_t)B * N * sizeof(float) + (size_t)B * (N - N / 4) * sizeof(int);   // rn [B][N] | merged [B][Ns]
}

template <typename T> static bool tome_width_ok(int C, int ld) {
  constexpr int EPC = 16 / sizeof(T);
  return C > 0 && C % EPC == 0 && ld % EPC == 0 && C / EPC <= 64 * tome::LN_MAXV;
}

template <int NK>
static int launch_match_mfma(const bf16* x, int ldx, int B, int W, int Nd, int Ns, const float* rn, int* node_idx, float* node_max,
                             hipStream_t s) {
  constexpr int lds = 2 * 32 * (NK * 32 + 16) + 2 * 32 * (int)sizeof(float);
  return af_launch_lds<tome::tome_match_mfma_kernel<NK>>(dim3((Ns + 127) / 128, B), dim3(256), lds, lds, s, x, ldx, W, Nd, Ns, rn,
                                                         node_idx, node_max);
}

template <typename T>
int af_launch_tome_match(const void* x_, int ldx, int B, int H, int W, int C, double ratio, int normalize, int* node_idx,
                         float* node_max, int* map, void* ws, hipStream_t s) {
  AfTomePlan pl;
  if (af_tome_plan(H, W, ratio, &pl)) return -1;
  if (!tome_width_ok<T>(C, ldx)) { af_set_error_msg("token merging: unsupported C=%d (row stride %d)", C, ldx); return -1; }
  if (B <= 0) return 0;
  if (!node_idx || !node_max || !map || !ws) { af_set_error_msg("token merging: null output or workspace"); return -1; }
  const T* x = reinterpret_cast<const T*>(x_);
  const int N = H * W, Nd = (int)pl.Nd, Ns = (int)pl.Ns;
  float* rn = reinterpret_cast<float*>(ws);
  int* merged = reinterpret_cast<int*>(rn + (size_t)B * N);
  if (normalize) {
    const long rows = (long)B * N;
    AfProfScope prof(AF_K_TOME_RNORM, s, 0.0, (double)rows * C * sizeof(T));
    hipLaunchKernelGGL((tome::tome_rnorm_kernel<T>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, ldx, rows, C, rn);
    HIP_CHECK_RET(hipGetLastError());
  }
  const float* rnp = normalize ? rn : nullptr;
  bool done = false;
  {
  AfProfScope prof(AF_K_TOME_MATCH, s, 2.0 * B * (double)Ns * Nd * C, (double)B * N * C * sizeof(T));
  if constexpr (std::is_same_v<T, bf16>) {
    done = true;
    int rc = 0;
    switch (C) {   // (the widths of the U-Net levels that merge: 320 / 640, and those of the narrow test model)
      case 64: rc = launch_match_mfma<4>(x, ldx, B, W, Nd, Ns, rnp, node_idx, node_max, s); break;
      case 128: rc = launch_match_mfma<8>(x, ldx, B, W, Nd, Ns, rnp, node_idx, node_max, s); break;
      case 256: rc = launch_match_mfma<16>(x, ldx, B, W, Nd, Ns, rnp, node_idx, node_max, s); break;
      case 320: rc = launch_match_mfma<20>(x, ldx, B, W, Nd, Ns, rnp, node_idx, node_max, s); break;
      case 640: rc = launch_match_mfma<40>(x, ldx, B, W, Nd, Ns, rnp, node_idx, node_max, s); break;
      default: done = false;
    }
    if (rc) return rc;
  }
  if (!done) {
    hipLaunchKernelGGL((tome::tome_match_plain_kernel<T>), dim3((Ns + 63) / 64, B), dim3(256), 0, s, x, ldx, W, Nd, Ns, C, rnp,
                       node_idx, node_max);
    HIP_CHECK_RET(hipGetLastError());
  }
  }
  {
    AfProfScope prof(AF_K_TOME_RANK, s, 0.0, (double)B * Ns * 8.0);
    hipLaunchKernelGGL(tome::tome_rank_kernel, dim3((Ns + 255) / 256, B), dim3(256), 0, s, node_max, Ns, (int)pl.r, merged);
    HIP_CHECK_RET(hipGetLastError());
  }
  AfProfScope prof(AF_K_TOME_MAP, s, 0.0, (double)B * (N + 2.0 * Ns) * 4.0);
  hipLaunchKernelGGL(tome::tome_map_kernel, dim3(B), dim3(256), 0, s, merged, node_idx, W, Nd, Ns, map);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

template <typename T>
int af_launch_tome_merge(const void* x, int ldx, const float* gamma, const float* beta, float eps, const int* map, int B, int N,
                         int Np, int C, void* y, int ldy, hipStream_t s) {
  if (!tome_width_ok<T>(C, ldx) || ldy % (16 / (int)sizeof(T))) { af_set_error_msg("token merge: unsupported C=%d", C); return -1; }
  if (N <= 0 || Np <= 0 || Np > N) { af_set_error_msg("token merge: %d rows from %d tokens", Np, N); return -1; }
  if ((size_t)((N + 255) & ~255) * sizeof(int) > 65536) { af_set_error_msg("token merge: %d tokens per sample exceed the 16384 the kernel holds", N); return -1; }
  if (gamma && !beta) { af_set_error_msg("token merge: gamma without beta"); return -1; }
  if (B <= 0) return 0;
  AfProfScope prof(AF_K_TOME_MERGE, s, 0.0, (double)B * ((double)N + Np) * C * sizeof(T));
  const int lds = ((N + 255) & ~255) * (int)sizeof(int);
  const dim3 grid((Np + tome::MERGE_ROWS - 1) / tome::MERGE_ROWS, B);
  const T* xp = reinterpret_cast<const T*>(x);
  T* yp = reinterpret_cast<T*>(y);
  switch ((C / (16 / (int)sizeof(T)) + 63) / 64) {   // vectors a lane holds
    case 1: return af_launch_lds<tome::tome_merge_kernel<T, 1>>(grid, dim3(256), 65536, lds, s, xp, ldx, gamma, beta, eps, map, N, Np, C, yp, ldy);
    case 2: return af_launch_lds<tome::tome_merge_kernel<T, 2>>(grid, dim3(256), 65536, lds, s, xp, ldx, gamma, beta, eps, map, N, Np, C, yp, ldy);
    case 3: return af_launch_lds<tome::tome_merge_kernel<T, 3>>(grid, dim3(256), 65536, lds, s, xp, ldx, gamma, beta, eps, map, N, Np, C, yp, ldy);
    case 4: return af_launch_lds<tome::tome_merge_kernel<T, 4>>(grid, dim3(256), 65536, lds, s, xp, ldx, gamma, beta, eps, map, N, Np, C, yp, ldy);
    default: return af_launch_lds<tome::tome_merge_kernel<T, 5>>(grid, dim3(256), 65536, lds, s, xp, ldx, gamma, beta, eps, map, N, Np, C, yp, ldy);
  }
}

template <typename T>
int af_launch_tome_unmerge_add(const void* o, int ldo, const void* res, int ldr, const int* map, int B, int N, int Np, int C,
                               void* y, int ldy, float* ln_stats_out, int ln_parts, hipStream_t s) {
  constexpr int EPC = 16 / sizeof(T);
  if (!tome_width_ok<T>(C, ldo) || ldr % EPC || ldy % EPC) { af_set_error_msg("token unmerge: unsupported C=%d", C); return -1; }
  if (N <= 0 || Np <= 0 || Np > N) { af_set_error_msg("token unmerge: %d rows for %d tokens", Np, N); return -1; }
  if (ln_stats_out && ln_parts <= 0) { af_set_error_msg("token unmerge: LayerNorm statistics without a part count"); return -1; }
  if (B <= 0) return 0;
  const long rows = (long)B * N;
  AfProfScope prof(AF_K_TOME_UNMERGE, s, 0.0, 3.0 * rows * C * sizeof(T));
  hipLaunchKernelGGL((tome::tome_unmerge_add_kernel<T>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s,
                     reinterpret_cast<const T*>(o), ldo, reinterpret_cast<const T*>(res), ldr, map, N, Np, rows, C,
                     reinterpret_cast<T*>(y), ldy, ln_stats_out, ln_parts);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

#define AF_TOME_INST(T)                                                                                                          \
  template int af_launch_tome_match<T>(const void*, int, int, int, int, int, double, int, int*, float*, int*, void*, hipStream_t); \
  template int af_launch_tome_merge<T>(const void*, int, const float*, const float*, float, const int*, int, int, int, int, void*, \
                                       int, hipStream_t);                                                                        \
  template int af_launch_tome_unmerge_add<T>(const void*, int, const void*, int, const int*, int, int, int, int, void*, int,      \
                                             float*, int, hipStream_t);
AF_TOME_INST(bf16)
AF_TOME_INST(float)
