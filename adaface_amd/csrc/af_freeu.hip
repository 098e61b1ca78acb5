// adaface_amd — FreeU (Si, Huang, Jiang, Liu, "FreeU: Free Lunch in Diffusion U-Net", CVPR 2024; the authors' LDM patch,
// Free_UNetModel.forward and Fourier_filter with threshold = 1), in place on the concatenation buffer of one output block:
// pixel rows [h (Ch channels) | skip (Cs channels)] with pitch ld = Ch + Cs, NHWC.
//
//   backbone, channels [0, Ch / 2):  version 1: x * b
//                                    version 2: x * ((b - 1) * mhat + 1), mhat = (m - min m) / (max m - min m) per sample,
//                                               m = the mean of a pixel over all Ch channels
//   [Ch / 2, Ch):                    neither read (version 1) nor ever written
//   skip, all Cs channels:           x + (s - 1) * low, low = the projection of the map onto the frequencies (ky, kx) in
//                                    {-1, 0}^2, which is what fftshift / 2 x 2 box / ifftshift / .real of the reference keep:
//       low(y, x) = 1 / (H W) [S0 + Cy cos ty + Sy sin ty + Cx cos tx + Sx sin tx + Cyx cos(ty + tx) + Syx sin(ty + tx)],
//       ty = 2 pi y / H, tx = 2 pi x / W, the seven sums over the map.  H, W >= 2.
//
// A workgroup is CV = 8 channel vectors (16 bytes each) x PL = 32 pixel lanes; a lane walks PPT = 8 pixels, 256 pixels a chunk.
//   H W <= 256: freeu_small_kernel -- sums (lane, wave butterfly, the four waves through LDS, all in a fixed order) and apply in
//               one launch, the map in registers between them.
//   larger:     freeu_sums_kernel writes one partial per chunk, [B][chunk][7][Cs]; freeu_apply_kernel adds them in ascending
//               chunk order.
//   version 2:  freeu_mean_kernel in front: m [B][H W] and one (min, max) per workgroup, combined by the consumer (min and max
//               do not depend on the order).
// No atomics: a sample's bits depend on nothing but that sample.  fp32 arithmetic on the stored values, one rounding.
#include "af_kernels.h"

namespace freeu {

constexpr int CV = 8;              // channel vectors of a workgroup (128 contiguous bytes of a pixel row)
constexpr int PL = 32;             // pixel lanes
constexpr int PPT = 8;             // pixels a lane walks
constexpr int CHUNK = PL * PPT;    // pixels of a workgroup
constexpr int NS = 7;              // sums per channel
constexpr int MEAN_PIX = 16;       // pixels of a freeu_mean_kernel workgroup (four per wave)
static_assert(CV * PL == 256 && AF_WAVE % CV == 0, "thread = pixel lane * CV + channel vector; a wave holds whole pixel lanes");

struct Args {
  void* cat;
  int ld, H, W, Ch;
  int nvh;                 // backbone vectors to scale, (Ch / 2) / EPV (0: the backbone is left alone)
  int nvs;                 // skip vectors to filter, Cs / EPV (0: the skip is left alone)
  int Cs;
  int version;
  float b;
  float sm1_hw;            // (s - 1) / (H W)
  const float* mean;       // version 2: [B][H W]
  const float* mm;         // version 2: [B][mm_n][2] (min, max)
  int mm_n;
  float* part;             // chunked form: [B][nchunk][7][Cs]
  int nchunk;
};

struct Trig { float cy, sy, cx, sx, cyx, syx; };
__device__ __forceinline__ Trig trig_of(int p, int H, int W) {
  const int y = p / W, x = p - y * W;
  const float ay = (float)(2 * y) / (float)H, ax = (float)(2 * x) / (float)W;   // angles in units of pi: exact at the quadrants
  Trig t;
  t.cy = cospif(ay); t.sy = sinpif(ay);
  t.cx = cospif(ax); t.sx = sinpif(ax);
  t.cyx = t.cy * t.cx - t.sy * t.sx;
  t.syx = t.sy * t.cx + t.cy * t.sx;
  return t;
}

// the column (in elements) of work vector wv: the scaled half of the backbone first, then the skip
__device__ __forceinline__ int col_of(int wv, int nvh, int Ch, int epv) { return wv < nvh ? wv * epv : Ch + (wv - nvh) * epv; }

template <typename T>
__device__ __forceinline__ void add_pixel(float (&acc)[NS][Vec16<T>::N], const Vec16<T>& v, const Trig& t) {
#pragma unroll
  for (int e = 0; e < Vec16<T>::N; ++e) {
    const float f = to_f32<T>(v.e[e]);
    acc[0][e] += f;
    acc[1][e] = fmaf(f, t.cy, acc[1][e]);
    acc[2][e] = fmaf(f, t.sy, acc[2][e]);
    acc[3][e] = fmaf(f, t.cx, acc[3][e]);
    acc[4][e] = fmaf(f, t.sx, acc[4][e]);
    acc[5][e] = fmaf(f, t.cyx, acc[5][e]);
    acc[6][e] = fmaf(f, t.syx, acc[6][e]);
  }
}

// The sums of the workgroup's pixels for every channel vector: butterfly over the 8 pixel lanes of a wave (every lane ends
// with the same value), then the four waves in ascending order.  red: [4][CV][NS * EPV] floats.  All threads call this.
template <int EPV>
__device__ __forceinline__ void block_sums(float (&acc)[NS][EPV], float* red, int tid) {
  const int cv = tid % CV, wave = tid / AF_WAVE;
#pragma unroll
  for (int k = 0; k < NS; ++k)
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
      float v = acc[k][e];
#pragma unroll
      for (int off = CV; off < AF_WAVE; off <<= 1) v += __shfl_xor(v, off, AF_WAVE);
      acc[k][e] = v;
    }
  if ((tid % AF_WAVE) < CV) {
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
      for (int e = 0; e < EPV; ++e) red[(wave * CV + cv) * (NS * EPV) + k * EPV + e] = acc[k][e];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NS; ++k)
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
      float v = red[cv * (NS * EPV) + k * EPV + e];
#pragma unroll
      for (int w = 1; w < 4; ++w) v += red[(w * CV + cv) * (NS * EPV) + k * EPV + e];
      acc[k][e] = v;
    }
}

// version 2: (min, max) of the sample's pixel means from the producer's per-workgroup pairs.  mmred: 8 floats.  All threads.
__device__ __forceinline__ float2 sample_minmax(const float* mm, int n, float* mmred, int tid) {
  float mn = INFINITY, mx = -INFINITY;
  for (int i = tid; i < n; i += 256) {
    mn = fminf(mn, mm[2 * i]);
    mx = fmaxf(mx, mm[2 * i + 1]);
  }
#pragma unroll
  for (int off = 1; off < AF_WAVE; off <<= 1) {
    mn = fminf(mn, __shfl_xor(mn, off, AF_WAVE));
    mx = fmaxf(mx, __shfl_xor(mx, off, AF_WAVE));
  }
  if (tid % AF_WAVE == 0) { mmred[2 * (tid / AF_WAVE)] = mn; mmred[2 * (tid / AF_WAVE) + 1] = mx; }
  __syncthreads();
  mn = fminf(fminf(mmred[0], mmred[2]), fminf(mmred[4], mmred[6]));
  mx = fmaxf(fmaxf(mmred[1], mmred[3]), fmaxf(mmred[5], mmred[7]));
  return float2{mn, mx};
}

// one pixel of one work vector: v -> its FreeU value.  coef: the seven sums times (s - 1) / (H W) (skip vectors)
template <typename T>
__device__ __forceinline__ void apply_pixel(Vec16<T>& v, bool backbone, float factor, const float (&coef)[NS][Vec16<T>::N],
                                            const Trig& t) {
#pragma unroll
  for (int e = 0; e < Vec16<T>::N; ++e) {
    const float f = to_f32<T>(v.e[e]);
    float r;
    if (backbone) {
      r = f * factor;
    } else {
      float low = coef[0][e];
      low = fmaf(coef[1][e], t.cy, low);
      low = fmaf(coef[2][e], t.sy, low);
      low = fmaf(coef[3][e], t.cx, low);
      low = fmaf(coef[4][e], t.sx, low);
      low = fmaf(coef[5][e], t.cyx, low);
      low = fmaf(coef[6][e], t.syx, low);
      r = f + low;
    }
    v.e[e] = from_f32<T>(r);
  }
}

// the backbone factor of pixel p (sample-relative) of sample b
__device__ __forceinline__ float backbone_factor(const Args& a, int b, int p, float2 mnmx) {
  if (a.version != 2) return a.b;
  const float m = a.mean[(long)b * a.H * a.W + p];
  return (a.b - 1.f) * ((m - mnmx.x) / (mnmx.y - mnmx.x)) + 1.f;
}

// H W <= CHUNK: grid (ceil(work vectors / CV), B)
template <typename T> __global__ __launch_bounds__(256) void freeu_small_kernel(Args a) {
  constexpr int EPV = Vec16<T>::N;
  __shared__ float red[4 * CV * NS * EPV];
  __shared__ float mmred[8];
  const int tid = threadIdx.x, cv = tid % CV, pl = tid / CV, b = blockIdx.y;
  const int HW = a.H * a.W, nwv = a.nvh + a.nvs;
  const int wv = blockIdx.x * CV + cv;
  const bool live = wv < nwv, backbone = wv < a.nvh;
  T* base = reinterpret_cast<T*>(a.cat) + (long)b * HW * a.ld + (live ? col_of(wv, a.nvh, a.Ch, EPV) : 0);
  Vec16<T> v[PPT];
  float acc[NS][EPV];
#pragma unroll
  for (int k = 0; k < NS; ++k)
#pragma unroll
    for (int e = 0; e < EPV; ++e) acc[k][e] = 0.f;
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int p = i * PL + pl;
    if (live && p < HW) {
      v[i].u = *reinterpret_cast<const uint4*>(base + (long)p * a.ld);
      if (!backbone) add_pixel<T>(acc, v[i], trig_of(p, a.H, a.W));
    }
  }
  if (a.nvs) {
    block_sums<EPV>(acc, red, tid);
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
      for (int e = 0; e < EPV; ++e) acc[k][e] *= a.sm1_hw;
  }
  float2 mnmx = float2{0.f, 1.f};
  if (a.version == 2 && a.nvh) mnmx = sample_minmax(a.mm + (long)b * a.mm_n * 2, a.mm_n, mmred, tid);
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int p = i * PL + pl;
    if (live && p < HW) {
      const float factor = backbone ? backbone_factor(a, b, p, mnmx) : 1.f;
      apply_pixel<T>(v[i], backbone, factor, acc, trig_of(p, a.H, a.W));
      *reinterpret_cast<uint4*>(base + (long)p * a.ld) = v[i].u;
    }
  }
}

// grid (ceil(skip vectors / CV), nchunk, B): the chunk's seven sums per skip channel -> part [B][nchunk][7][Cs]
template <typename T> __global__ __launch_bounds__(256) void freeu_sums_kernel(Args a) {
  constexpr int EPV = Vec16<T>::N;
  __shared__ float red[4 * CV * NS * EPV];
  const int tid = threadIdx.x, cv = tid % CV, pl = tid / CV, chunk = blockIdx.y, b = blockIdx.z;
  const int HW = a.H * a.W;
  const int sv = blockIdx.x * CV + cv;      // skip vector
  const bool live = sv < a.nvs;
  const T* base = reinterpret_cast<const T*>(a.cat) + (long)b * HW * a.ld + a.Ch + (live ? sv * EPV : 0);
  float acc[NS][EPV];
#pragma unroll
  for (int k = 0; k < NS; ++k)
#pragma unroll
    for (int e = 0; e < EPV; ++e) acc[k][e] = 0.f;
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int p = chunk * CHUNK + i * PL + pl;
    if (live && p < HW) {
      Vec16<T> v;
      v.u = *reinterpret_cast<const uint4*>(base + (long)p * a.ld);
      add_pixel<T>(acc, v, trig_of(p, a.H, a.W));
    }
  }
  block_sums<EPV>(acc, red, tid);
  if (live && pl == 0) {
    float* out = a.part + ((long)b * a.nchunk + chunk) * NS * a.Cs + sv * EPV;
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
      for (int e = 0; e < EPV; ++e) out[(long)k * a.Cs + e] = acc[k][e];
  }
}

// grid (ceil(work vectors / CV), nchunk, B)
template <typename T> __global__ __launch_bounds__(256) void freeu_apply_kernel(Args a) {
  constexpr int EPV = Vec16<T>::N;
  __shared__ float coefs[CV * NS * EPV];
  __shared__ float mmred[8];
  const int tid = threadIdx.x, cv = tid % CV, pl = tid / CV, chunk = blockIdx.y, b = blockIdx.z;
  const int HW = a.H * a.W, nwv = a.nvh + a.nvs;
  const int wv = blockIdx.x * CV + cv;
  const bool live = wv < nwv, backbone = wv < a.nvh;
  // the sample's sums of this workgroup's skip channels: a (vector, sum, element) per thread and turn, chunks in ascending order
  for (int o = tid; o < CV * NS * EPV; o += 256) {
    const int ocv = o / (NS * EPV), k = (o / EPV) % NS, e = o % EPV;
    const int owv = blockIdx.x * CV + ocv;
    float v = 0.f;
    if (owv >= a.nvh && owv < nwv) {
      const float* src = a.part + (long)b * a.nchunk * NS * a.Cs + (long)k * a.Cs + (owv - a.nvh) * EPV + e;
      for (int c = 0; c < a.nchunk; ++c) v += src[(long)c * NS * a.Cs];
    }
    coefs[o] = v * a.sm1_hw;
  }
  __syncthreads();
  float coef[NS][EPV];
#pragma unroll
  for (int k = 0; k < NS; ++k)
#pragma unroll
    for (int e = 0; e < EPV; ++e) coef[k][e] = coefs[cv * (NS * EPV) + k * EPV + e];
  float2 mnmx = float2{0.f, 1.f};
  if (a.version == 2 && a.nvh) mnmx = sample_minmax(a.mm + (long)b * a.mm_n * 2, a.mm_n, mmred, tid);
  T* base = reinterpret_cast<T*>(a.cat) + (long)b * HW * a.ld + (live ? col_of(wv, a.nvh, a.Ch, EPV) : 0);
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int p = chunk * CHUNK + i * PL + pl;
    if (live && p < HW) {
      Vec16<T> v;
      v.u = *reinterpret_cast<const uint4*>(base + (long)p * a.ld);
      const float factor = backbone ? backbone_factor(a, b, p, mnmx) : 1.f;
      apply_pixel<T>(v, backbone, factor, coef, trig_of(p, a.H, a.W));
      *reinterpret_cast<uint4*>(base + (long)p * a.ld) = v.u;
    }
  }
}

// version 2, grid (ceil(H W / MEAN_PIX), B): a wave per pixel, four pixels per wave -> mean [B][H W], mm [B][gridDim.x][2]
template <typename T>
__global__ __launch_bounds__(256) void freeu_mean_kernel(const T* __restrict__ cat, int ld, int HW, int Ch, float* __restrict__ mean,
                                                         float* __restrict__ mm) {
  constexpr int EPV = Vec16<T>::N;
  __shared__ float mmred[8];
  const int tid = threadIdx.x, lane = tid % AF_WAVE, wave = tid / AF_WAVE, b = blockIdx.y;
  const int nv = Ch / EPV;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = 0; i < MEAN_PIX / 4; ++i) {
    const int p = blockIdx.x * MEAN_PIX + wave * (MEAN_PIX / 4) + i;
    if (p >= HW) break;                       // (wave-uniform)
    const T* row = cat + ((long)b * HW + p) * ld;
    float s = 0.f;
    for (int v = lane; v < nv; v += AF_WAVE) {
      Vec16<T> x;
      x.u = *reinterpret_cast<const uint4*>(row + v * EPV);
#pragma unroll
      for (int e = 0; e < EPV; ++e) s += to_f32<T>(x.e[e]);
    }
#pragma unroll
    for (int off = 1; off < AF_WAVE; off <<= 1) s += __shfl_xor(s, off, AF_WAVE);
    const float m = s / (float)Ch;
    if (lane == 0) mean[(long)b * HW + p] = m;
    mn = fminf(mn, m);
    mx = fmaxf(mx, m);
  }
  if (lane == 0) { mmred[2 * wave] = mn; mmred[2 * wave + 1] = mx; }
  __syncthreads();
  if (tid == 0) {
    float* o = mm + ((long)b * gridDim.x + blockIdx.x) * 2;
    o[0] = fminf(fminf(mmred[0], mmred[2]), fminf(mmred[4], mmred[6]));
    o[1] = fmaxf(fmaxf(mmred[1], mmred[3]), fmaxf(mmred[5], mmred[7]));
  }
}

}  // namespace freeu

// ---- host -----------------------------------------------------------------------------------------------------------------
int af_plan_freeu(int H, int W, int Ch, int Cs, int version, AfFreeuPlan* pl) {
  *pl = AfFreeuPlan{AF_FREEUK_REFUSED, 0, 0, 0};
  if (version != 1 && version != 2) { af_set_error_msg("FreeU: version %d is neither 1 nor 2", version); return -1; }
  if (H < 2 || W < 2) {
    af_set_error_msg("FreeU: the Fourier filter needs map sides >= 2, got %d x %d", H, W);
    return -1;
  }
  if ((long)H * W > (1L << 22)) { af_set_error_msg("FreeU: a %d x %d map is beyond the kernels' pixel index", H, W); return -1; }
  if (Ch <= 0 || Ch % 16) { af_set_error_msg("FreeU: %d backbone channels (a positive multiple of 16)", Ch); return -1; }
  if (Cs <= 0 || Cs % 8) { af_set_error_msg("FreeU: %d skip channels (a positive multiple of 8)", Cs); return -1; }
  const int HW = H * W;
  pl->nchunk = (HW + freeu::CHUNK - 1) / freeu::CHUNK;
  pl->kernel = pl->nchunk == 1 ? AF_FREEUK_SINGLE : AF_FREEUK_CHUNKED;
  pl->launches = (pl->nchunk == 1 ? 1 : 2) + (version == 2 ? 1 : 0);
  pl->part_bytes = pl->nchunk == 1 ? 0 : (long)pl->nchunk * freeu::NS * Cs * (long)sizeof(float);
  return 0;
}

static size_t freeu_round(size_t n) { return (n + 255) & ~(size_t)255; }
static int freeu_mean_blocks(int HW) { return (HW + freeu::MEAN_PIX - 1) / freeu::MEAN_PIX; }

size_t af_freeu_ws_bytes(int B, int H, int W, int Ch, int Cs, int version) {
  AfFreeuPlan pl;
  if (af_plan_freeu(H, W, Ch, Cs, version, &pl)) return 0;
  size_t n = freeu_round((size_t)B * pl.part_bytes);
  if (version == 2) n += freeu_round((size_t)B * H * W * sizeof(float)) + freeu_round((size_t)B * freeu_mean_blocks(H * W) * 2 * sizeof(float));
  return n + 256;
}

template <typename T>
int af_launch_freeu(void* cat, int ld, int B, int H, int W, int Ch, int Cs, int version, float b, float s, bool backbone,
                    bool skip, void* ws, hipStream_t stream) {
  constexpr int EPV = 16 / (int)sizeof(T);
  AfFreeuPlan pl;
  if (af_plan_freeu(H, W, Ch, Cs, version, &pl)) return -1;
  if (ld < Ch + Cs || ld % EPV) { af_set_error_msg("FreeU: pixel pitch %d for %d + %d channels", ld, Ch, Cs); return -1; }
  if (!(b >= 1.f && b <= 2.f) || !(s >= 0.f && s <= 1.f)) { af_set_error_msg("FreeU: b %g outside [1, 2] or s %g outside [0, 1]", b, s); return -1; }
  if (b == 1.f) backbone = false;     // (x * 1 and x + 0 * low are x: the bits stay and so may the launch)
  if (s == 1.f) skip = false;
  if (B <= 0 || (!backbone && !skip)) return 0;
  if (!cat || !ws) { af_set_error_msg("FreeU: null tensor or workspace"); return -1; }
  const int HW = H * W;
  freeu::Args a;
  a.cat = cat; a.ld = ld; a.H = H; a.W = W; a.Ch = Ch; a.Cs = Cs;
  a.nvh = backbone ? (Ch / 2) / EPV : 0;
  a.nvs = skip ? Cs / EPV : 0;
  a.version = version;
  a.b = b;
  a.sm1_hw = (s - 1.f) / (float)HW;
  a.nchunk = pl.nchunk;
  char* w = reinterpret_cast<char*>(ws);
  a.part = reinterpret_cast<float*>(w);
  w += freeu_round((size_t)B * pl.part_bytes);
  float* mean = reinterpret_cast<float*>(w);
  w += freeu_round((size_t)B * HW * sizeof(float));
  float* mm = reinterpret_cast<float*>(w);
  a.mean = mean; a.mm = mm; a.mm_n = freeu_mean_blocks(HW);
  const double esz = (double)sizeof(T);
  if (version == 2 && backbone) {
    AfProfScope prof(AF_K_FREEU_MEAN, stream, 0.0, (double)B * HW * Ch * esz);
    hipLaunchKernelGGL((freeu::freeu_mean_kernel<T>), dim3(a.mm_n, B), dim3(256), 0, stream, reinterpret_cast<const T*>(cat), ld, HW,
                       Ch, mean, mm);
    HIP_CHECK_RET(hipGetLastError());
  }
  const int nwv = a.nvh + a.nvs;
  const double touched = 2.0 * B * HW * (double)nwv * 16.0;
  if (pl.kernel == AF_FREEUK_SINGLE) {
    AfProfScope prof(AF_K_FREEU_SMALL, stream, 0.0, touched);
    hipLaunchKernelGGL((freeu::freeu_small_kernel<T>), dim3((nwv + freeu::CV - 1) / freeu::CV, B), dim3(256), 0, stream, a);
    HIP_CHECK_RET(hipGetLastError());
    return 0;
  }
  if (skip) {
    AfProfScope prof(AF_K_FREEU_SUMS, stream, 0.0, (double)B * HW * Cs * esz);
    hipLaunchKernelGGL((freeu::freeu_sums_kernel<T>), dim3((a.nvs + freeu::CV - 1) / freeu::CV, pl.nchunk, B), dim3(256), 0, stream, a);
    HIP_CHECK_RET(hipGetLastError());
  }
  AfProfScope prof(AF_K_FREEU_APPLY, stream, 0.0, touched);
  hipLaunchKernelGGL((freeu::freeu_apply_kernel<T>), dim3((nwv + freeu::CV - 1) / freeu::CV, pl.nchunk, B), dim3(256), 0, stream, a);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

#define AF_FREEU_INST(T) \
  template int af_launch_freeu<T>(void*, int, int, int, int, int, int, int, float, float, bool, bool, void*, hipStream_t);
AF_FREEU_INST(bf16)
AF_FREEU_INST(float)
AF_FREEU_INST(f16)
