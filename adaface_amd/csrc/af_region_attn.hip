// Regional prompts (attention couple): per-region cross-attention in one pass.  DESIGN 2u.
//
// The context of a sample is R segments of T keys (segment 0 = the base prompt) and a weight map m[b][r][H][W] >= 0 at the
// latent resolution says which regions a pixel listens to.  At a site whose map is (H / f, W / f), f in {1, 2, 4, 8}:
//     a_r(p) = mean of m_r over the f x f box of p,   s(p) = sum_r a_r(p) (r ascending),
//     w_r(p) = a_r(p) / s(p) where s(p) > 0, else w_0 = 1 and w_{r > 0} = 0,
//     o(p)   = sum_{r : w_r(p) > 0} w_r(p) softmax(q_p K_r^T dh^-1/2) V_r        (exact softmax per region, fp32 sum)
// Regions with w_r(p) = 0 are SELECTED OUT, never multiplied by zero: a NaN in the K / V rows of region r does not reach p.
//
//   * region_weights_kernel: one launch per af_set_regions -> the four-level pyramid w [level][Bf][R][N_level] (fp32) and one
//     word of active-region bits per (level, sample, block of 32 queries): bit r = some w_r > 0 in the block.  A pixel is a
//     thread; its box is summed row by row, left to right, so the result does not depend on the launch.
//   * region_attn_kernel<T, DH>: the shape of xs::xattn_short_kernel (af_attention.hip) -- one wave per head, four heads per
//     workgroup, blocks of 32 queries, S^T = K_r Q^T so that a query's <= 96 scores sit in one lane -- but K and V^T fragments
//     are read per ACTIVE region of the block (a wave-uniform walk over the block's bits) and the normalised region outputs
//     are folded into one fp32 accumulator that is stored once.  Keys >= T of a segment are masked to -inf: the rows behind
//     segment r are segment r + 1's keys, not padding.  The softmax denominator is the fp32 sum of the ROUNDED probabilities
//     (what the PV MFMA multiplies), so a region's output is a convex combination of its V rows.
//   * region_pack_vt_kernel<T>: V of the cached [Bf][R T][2C] tensor as per-segment V^T operand fragments (batch Bf R), in the
//     key order in which the S^T accumulator comes back as the B operand (as xs::pack_vt_kernel, without its ones row and for
//     every head dim and both 16-bit types).
//   * region_combine_kernel<T>: the composition's weighted select-sum of R attention outputs, 16-byte accesses.
#include "af_device.h"
#include "af_kernels.h"
#include <math.h>

namespace rg {
constexpr int NKB = 3, TMAX = 32 * NKB;            // key blocks of 32 per segment; keys >= T are masked
template <int DH> struct Cfg {
  static constexpr int KS = (DH + 15) / 16;        // 16-wide k steps of QK^T (dh 40: 3, the last half zero)
  static constexpr int DB = (DH + 31) / 32;        // 32-row blocks of O^T
  static constexpr int VSTEPS = 2 * NKB;           // 16-key k steps of PV
};
inline long pack_elems_per_head(int dh) { return (long)((dh + 31) / 32) * (2 * NKB) * 2 * 32 * 8; }

// ---- the weight pyramid ----
struct WeightsParams {
  const float* m;        // [Bf][R][H][W]
  float* pyr;            // [level][Bf][R][N_level]
  unsigned* bits;        // [level][Bf][nblk_level]
  int Bf, R, H, W;
  long w_off[4], b_off[4];
  int cstart[5];         // first workgroup of a level (256 pixels of one sample per workgroup)
};

__global__ __launch_bounds__(256) void region_weights_kernel(const WeightsParams p) {
  int lvl = 0;
#pragma unroll
  for (int l = 1; l < 4; ++l)
    if ((int)blockIdx.x >= p.cstart[l]) lvl = l;
  const int f = 1 << lvl, Hl = p.H >> lvl, Wl = p.W >> lvl, N = Hl * Wl;
  const int chunks = (N + 255) / 256, nblk = (N + 31) / 32;
  const int rel = (int)blockIdx.x - p.cstart[lvl];
  const int b = rel / chunks, chunk = rel - b * chunks;
  const int px = chunk * 256 + (int)threadIdx.x;
  const bool ok = px < N;
  const int y = ok ? px / Wl : 0, x = ok ? px - y * Wl : 0;
  const float inv_area = 1.0f / (float)(f * f);   // (a power of two: the scale is exact)
  float a[AF_REGION_MAX];
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < AF_REGION_MAX; ++r) {
    a[r] = 0.f;
    if (r < p.R && ok) {
      const float* src = p.m + (((long)b * p.R + r) * p.H + (long)y * f) * p.W + (long)x * f;
      float acc = 0.f;
      for (int dy = 0; dy < f; ++dy)
        for (int dx = 0; dx < f; ++dx) acc += src[(long)dy * p.W + dx];
      a[r] = acc * inv_area;
      s += a[r];
    }
  }
  unsigned lo = 0, hi = 0;
#pragma unroll
  for (int r = 0; r < AF_REGION_MAX; ++r) {
    if (r < p.R) {   // (uniform)
      const float w = s > 0.f ? __fdiv_rn(a[r], s) : (r == 0 ? 1.0f : 0.0f);
      if (ok) p.pyr[p.w_off[lvl] + ((long)b * p.R + r) * N + px] = w;
      const unsigned long long act = __ballot(ok && w > 0.f);
      lo |= (unsigned)((act & 0xffffffffull) != 0) << r;
      hi |= (unsigned)((act >> 32) != 0) << r;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    const int blk = px >> 5;   // (px of lane 0: a multiple of 64)
    unsigned* dst = p.bits + p.b_off[lvl] + (long)b * nblk;
    if (blk < nblk) dst[blk] = lo;
    if (blk + 1 < nblk) dst[blk + 1] = hi;
  }
}

// ---- V^T fragments per (sample, segment, head): vt[b R + r][head][db][ks][h][l31][8] ----
template <typename T>
__global__ __launch_bounds__(256) void region_pack_vt_kernel(const T* __restrict__ v, int ldv, long bsv, int Tk, int R, int H,
                                                             int dh, long total, T* __restrict__ vt) {
  const int DB = (dh + 31) / 32;
  constexpr int VSTEPS = 2 * NKB;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    long r = i;
    const int j = (int)(r & 7); r >>= 3;
    const int l31 = (int)(r & 31); r >>= 5;
    const int h = (int)(r & 1); r >>= 1;
    const int ks = (int)(r % VSTEPS); r /= VSTEPS;
    const int db = (int)(r % DB); r /= DB;
    const int head = (int)(r % H); r /= H;
    const int seg = (int)(r % R);
    const long b = r / R;
    const int d = db * 32 + l31;
    const int key = 16 * ks + 8 * (j >> 2) + 4 * h + (j & 3);
    T val = (T)0.f;
    if (d < dh && key < Tk) val = v[b * bsv + ((long)seg * Tk + key) * ldv + head * dh + d];
    vt[i] = val;
  }
}

// ---- the fused kernel ----
struct AttnParams {
  const void* q; const void* k; void* o;   // T; k: the cached key list, R segments of Tk rows per sample
  const void* vt;                          // region_pack_vt_kernel's fragments
  const float* w;                          // [B][R][Nq], this site's level of the pyramid
  const unsigned* bits;                    // [B][nblk]
  int ldq, ldk, ldo;
  long bsq, bsk, bso;
  int Nq, Tk, R, H, nblk;
  float scale;
};

template <typename T, int DH>
__global__ __launch_bounds__(256) void region_attn_kernel(const AttnParams p, int bpw) {
  using C = Cfg<DH>;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int head = blockIdx.y * 4 + wave, b = blockIdx.z;
  if (head >= p.H) return;                                          // (wave-uniform; no barrier in this kernel)
  const T* Q = reinterpret_cast<const T*>(p.q) + (long)b * p.bsq + head * DH;
  const T* K = reinterpret_cast<const T*>(p.k) + (long)b * p.bsk + head * DH;
  T* O = reinterpret_cast<T*>(p.o) + (long)b * p.bso + head * DH;
  const float sl2 = p.scale * 1.44269504088896340736f;
  constexpr long PACK = (long)C::DB * C::VSTEPS * 2 * 32 * 8;      // elements per (sample, segment, head)
  const int blk0 = blockIdx.x * bpw, blk1 = blk0 + bpw < p.nblk ? blk0 + bpw : p.nblk;
  for (int blk = blk0; blk < blk1; ++blk) {
    const unsigned act = __builtin_amdgcn_readfirstlane(p.bits[(long)b * p.nblk + blk]);
    const int q = blk * 32 + l31;
    uint4 qf[C::KS];
#pragma unroll
    for (int s = 0; s < C::KS; ++s) {
      const int d0 = 16 * s + 8 * h;
      qf[s] = make_uint4(0, 0, 0, 0);
      if (q < p.Nq && d0 < DH) qf[s] = *reinterpret_cast<const uint4*>(Q + (long)q * p.ldq + d0);
    }
    f32x16 acc[C::DB];
#pragma unroll
    for (int db = 0; db < C::DB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[db][r] = 0.f;
    for (int r = 0; r < p.R; ++r) {
      if (!((act >> r) & 1u)) continue;                             // (wave-uniform: the block's active regions only)
      const float wr = q < p.Nq ? p.w[((long)b * p.R + r) * p.Nq + q] : 0.f;
      const T* Kr = K + (long)r * p.Tk * p.ldk;
      // ---- S^T = K_r Q^T; keys >= Tk are the next segment's (or nothing): never loaded, masked ----
      f32x16 sc[NKB];
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        if (32 * kb < p.Tk) {
#pragma unroll
          for (int i = 0; i < 16; ++i) sc[kb][i] = 0.f;
          const int key = 32 * kb + l31;
#pragma unroll
          for (int s = 0; s < C::KS; ++s) {
            const int d0 = 16 * s + 8 * h;
            uint4 kf = make_uint4(0, 0, 0, 0);
            if (key < p.Tk && d0 < DH) kf = *reinterpret_cast<const uint4*>(Kr + (long)key * p.ldk + d0);
            Mma<T>::step(kf, qf[s], sc[kb]);
          }
          if (32 * kb + 32 > p.Tk) {
#pragma unroll
            for (int i = 0; i < 16; ++i)
              if (32 * kb + acc_row(i, h) >= p.Tk) sc[kb][i] = -INFINITY;
          }
        } else {
#pragma unroll
          for (int i = 0; i < 16; ++i) sc[kb][i] = -INFINITY;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sc[kb][i]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float msl = mx * sl2;
      // ---- P, rounded to the storage type, and the sum of exactly those values ----
      uint4 pb[NKB][2];
      float l = 0.f;
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          Vec16<T> v;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            v.e[j] = from_f32<T>(__builtin_amdgcn_exp2f(fmaf(sc[kb][8 * s2 + j], sl2, -msl)));
            l += to_f32<T>(v.e[j]);
          }
          pb[kb][s2] = v.u;
        }
      l += __shfl_xor(l, 32, 64);
      const float c = wr * (1.0f / l);
      const bool take = wr > 0.f;
      // ---- O_r^T = V_r^T P^T, folded into the block's accumulator by selection ----
      const uint4* vp = reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(p.vt) + (((long)b * p.R + r) * p.H + head) * PACK);
#pragma unroll
      for (int db = 0; db < C::DB; ++db) {
        f32x16 o;
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = 0.f;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
          if (32 * kb < p.Tk) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) Mma<T>::step(vp[((db * C::VSTEPS + 2 * kb + s2) * 2 + h) * 32 + l31], pb[kb][s2], o);
          }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[db][i] += take ? c * o[i] : 0.f;
      }
    }
#pragma unroll
    for (int db = 0; db < C::DB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int dd = 32 * db + 8 * g + 4 * h;
        if (dd < DH) {
          Quad<T> ov;
#pragma unroll
          for (int e = 0; e < 4; ++e) ov.e[e] = from_f32<T>(acc[db][4 * g + e]);
          if (q < p.Nq) ov.store(O + (long)q * p.ldo + dd);
        }
      }
  }
}

// ---- the composition's combine: out[row] = sum_{r : w_r > 0} w_r src_r[row], fp32, r ascending ----
template <typename T>
__global__ __launch_bounds__(256) void region_combine_kernel(const T* __restrict__ src, long rs, const float* __restrict__ w,
                                                             T* __restrict__ out, int ldo, long rows, int Nq, int Cn, int R) {
  constexpr int EPV = 16 / sizeof(T);
  const int vpr = Cn / EPV;
  const long total = rows * vpr;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = i / vpr;
    const int v = (int)(i - row * vpr);
    const long b = row / Nq;
    const int q = (int)(row - b * Nq);
    float acc[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) acc[e] = 0.f;
    for (int r = 0; r < R; ++r) {
      const float wr = w[(b * R + r) * Nq + q];
      if (wr > 0.f) {
        Vec16<T> x;
        x.u = *reinterpret_cast<const uint4*>(src + r * rs + row * Cn + (long)v * EPV);
#pragma unroll
        for (int e = 0; e < EPV; ++e) acc[e] += wr * to_f32<T>(x.e[e]);
      }
    }
    Vec16<T> y;
#pragma unroll
    for (int e = 0; e < EPV; ++e) y.e[e] = from_f32<T>(acc[e]);
    *reinterpret_cast<uint4*>(out + row * ldo + (long)v * EPV) = y.u;
  }
}
}  // namespace rg

// ----------------------------------------------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------------------------------------------
std::atomic<long> g_af_region_attn_launches{0};

int af_region_layout(int Bf, int R, int H, int W, AfRegionLayout* L) {
  if (Bf <= 0 || R < 1 || R > AF_REGION_MAX || H <= 0 || W <= 0 || H % 8 || W % 8) {
    af_set_error_msg("regions: %d samples, %d regions, a %d x %d map (1 .. %d regions; map sides multiples of 8)", Bf, R, H, W,
                     AF_REGION_MAX);
    return -1;
  }
  long wo = 0, bo = 0;
  for (int l = 0; l < 4; ++l) {
    const long N = (long)(H >> l) * (W >> l);
    if (N > 0x3fffffffL) { af_set_error_msg("regions: a %d x %d map is beyond one launch", H, W); return -1; }
    L->N[l] = (int)N;
    L->nblk[l] = (int)((N + 31) / 32);
    L->w_off[l] = wo;
    L->b_off[l] = bo;
    wo += (long)Bf * R * N;
    bo += (long)Bf * L->nblk[l];
  }
  L->w_floats = wo;
  L->b_words = bo;
  return 0;
}

int af_launch_region_weights(const float* m, int Bf, int R, int H, int W, float* pyr, unsigned* bits, hipStream_t stream) {
  AfRegionLayout L;
  if (af_region_layout(Bf, R, H, W, &L)) return -1;
  if (!m || !pyr || !bits) { af_set_error_msg("regions: null argument"); return -1; }
  rg::WeightsParams p;
  p.m = m; p.pyr = pyr; p.bits = bits; p.Bf = Bf; p.R = R; p.H = H; p.W = W;
  long blocks = 0;
  for (int l = 0; l < 4; ++l) {
    p.w_off[l] = L.w_off[l];
    p.b_off[l] = L.b_off[l];
    p.cstart[l] = (int)blocks;
    blocks += (long)Bf * ((L.N[l] + 255) / 256);
    if (blocks > 0x7fffffffL) { af_set_error_msg("regions: %d samples of %d x %d are beyond one launch", Bf, H, W); return -1; }
  }
  p.cstart[4] = (int)blocks;
  AfProfScope prof(AF_K_OTHER, stream, 0.0, 0.0);
  hipLaunchKernelGGL(rg::region_weights_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

static bool region_fused_dh(int dh) { return dh == 32 || dh == 40 || dh == 64 || dh == 80 || dh == 128 || dh == 160; }

int af_plan_region_attention(AfStorage st, int dh, int T, int R) {
  if (R < 1 || R > AF_REGION_MAX || T < 1) return AF_RGK_REFUSED;
  switch (dh) {     // (the head dims of af_plan_attention: the composition runs on those kernels)
    case 8: case 16: case 32: case 40: case 64: case 80: case 128: case 160: break;
    default: return AF_RGK_REFUSED;
  }
  if (g_af_knobs.region_fused && st != AF_ST_F32 && T <= rg::TMAX && region_fused_dh(dh)) return AF_RGK_FUSED;
  return AF_RGK_COMPOSE;
}

template <typename T> long af_region_pack_elems(int B, int R, int H, int dh, int Tk) {
  if (std::is_same_v<T, float> || Tk < 1 || Tk > rg::TMAX || !region_fused_dh(dh)) return 0;
  return (long)B * R * H * rg::pack_elems_per_head(dh);
}

template <typename T>
int af_launch_region_pack(const void* v, int ldv, long bsv, int Tk, int R, int H, int dh, int B, void* vt, hipStream_t stream) {
  if constexpr (std::is_same_v<T, float>) {
    af_set_error_msg("regions: the fused kernel has no f32 form");
    return -1;
  } else {
    const long total = af_region_pack_elems<T>(B, R, H, dh, Tk);
    if (total <= 0 || !v || !vt) { af_set_error_msg("regions: no V^T pack for dh %d, %d keys per segment", dh, Tk); return -1; }
    unsigned blocks = (unsigned)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL((rg::region_pack_vt_kernel<T>), dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const T*>(v), ldv, bsv,
                       Tk, R, H, dh, total, reinterpret_cast<T*>(vt));
    HIP_CHECK_RET(hipGetLastError());
    return 0;
  }
}

template <typename T, int DH> static int launch_region_attn(const AfRegionAttnArgs& a, hipStream_t stream) {
  rg::AttnParams p;
  p.q = a.q; p.k = a.k; p.o = a.o; p.vt = a.vt; p.w = a.w; p.bits = a.bits;
  p.ldq = a.ldq; p.ldk = a.ldk; p.ldo = a.ldo; p.bsq = a.bsq; p.bsk = a.bsk; p.bso = a.bso;
  p.Nq = a.Nq; p.Tk = a.T; p.R = a.R; p.H = a.heads; p.nblk = (a.Nq + 31) / 32; p.scale = a.scale;
  // blocks of 32 queries per wave: about one round of workgroups over the chip, as launch_xattn_short
  const long wave_blocks = (long)a.B * a.heads * p.nblk;
  int bpw = (int)((wave_blocks + 2047) / 2048);
  if (bpw < 1) bpw = 1;
  if (bpw > 16) bpw = 16;
  const dim3 grid((p.nblk + bpw - 1) / bpw, (a.heads + 3) / 4, a.B);
  hipLaunchKernelGGL((rg::region_attn_kernel<T, DH>), grid, dim3(256), 0, stream, p, bpw);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

template <typename T> int af_launch_region_attention(const AfRegionAttnArgs& a, hipStream_t stream) {
  if constexpr (std::is_same_v<T, float>) {
    af_set_error_msg("regions: the fused kernel has no f32 form");
    return -1;
  } else {
    if (af_plan_region_attention(StorageOf<T>::value, a.dh, a.T, a.R) == AF_RGK_REFUSED || a.T > rg::TMAX || !region_fused_dh(a.dh) ||
        !a.q || !a.k || !a.o || !a.vt || !a.w || !a.bits || a.ldq % 8 || a.ldk % 8 || a.ldo % 4 || a.bsq % 8 || a.bsk % 8 ||
        a.bso % 4 || a.heads <= 0 || a.B > 65535 || (a.heads + 3) / 4 > 65535) {
      af_set_error_msg("regions: no fused kernel for head dim %d, %d regions of %d keys, %d heads, row strides %d / %d / %d", a.dh, a.R,
                       a.T, a.heads, a.ldq, a.ldk, a.ldo);
      return -1;
    }
    if (a.Nq <= 0 || a.B <= 0) return 0;
    AfProfScope prof(AF_K_REGION_ATTN + (a.level >= 0 && a.level < 4 ? a.level : 0), stream, 4.0 * a.B * a.heads * (double)a.Nq * a.T * a.dh,
                     (2.0 * a.Nq + 2.0 * a.R * a.T) * a.B * a.heads * a.dh * sizeof(T));
    int rc = -1;
    switch (a.dh) {
      case 32: rc = launch_region_attn<T, 32>(a, stream); break;
      case 40: rc = launch_region_attn<T, 40>(a, stream); break;
      case 64: rc = launch_region_attn<T, 64>(a, stream); break;
      case 80: rc = launch_region_attn<T, 80>(a, stream); break;
      case 128: rc = launch_region_attn<T, 128>(a, stream); break;
      case 160: rc = launch_region_attn<T, 160>(a, stream); break;
    }
    if (rc == 0) ++g_af_region_attn_launches;
    return rc;
  }
}

template <typename T>
int af_launch_region_combine(const void* src, long rs, const float* w, void* out, int ldo, int B, int Nq, int Cn, int R,
                             hipStream_t stream) {
  constexpr int EPV = 16 / sizeof(T);
  if (!src || !w || !out || R < 1 || R > AF_REGION_MAX || Cn <= 0 || Cn % EPV || ldo % EPV || ldo < Cn || rs % EPV ||
      (reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out)) % 16) {
    af_set_error_msg("regions: combine of %d outputs with %d channels, output pitch %d (whole 16-byte vectors, aligned)", R, Cn, ldo);
    return -1;
  }
  if (B <= 0 || Nq <= 0) return 0;
  const long rows = (long)B * Nq, total = rows * (Cn / EPV);
  unsigned blocks = (unsigned)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
  AfProfScope prof(AF_K_REGION_COMBINE, stream, 0.0, (double)(R + 1) * rows * Cn * sizeof(T));
  hipLaunchKernelGGL((rg::region_combine_kernel<T>), dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const T*>(src), rs, w,
                     reinterpret_cast<T*>(out), ldo, rows, Nq, Cn, R);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

#define AF_REGION_INST(T)                                                                                                     \
  template long af_region_pack_elems<T>(int, int, int, int, int);                                                             \
  template int af_launch_region_pack<T>(const void*, int, long, int, int, int, int, int, void*, hipStream_t);                 \
  template int af_launch_region_attention<T>(const AfRegionAttnArgs&, hipStream_t);                                           \
  template int af_launch_region_combine<T>(const void*, long, const float*, void*, int, int, int, int, int, hipStream_t);
AF_REGION_INST(bf16)
AF_REGION_INST(f16)
AF_REGION_INST(float)
