// adaface_amd — hires fix: separable 2-D resampling of fp32 planes from tap tables, the one host function that
// states the filters (nearest-exact, bilinear and bicubic as torch.nn.functional.interpolate with align_corners=False; lanczos3
// as Pillow's Image.resize(..., LANCZOS)), and the plan that owns a size pair's tables.  Upscaling only.  A translation unit of
// its own: no other kernel is touched by it.
#include "../../include/adaface_hip.h"
#include "af_kernels.h"
#include <cmath>
#include <vector>

std::atomic<long> g_af_resample2d_launches{0};

// ---------------------------------------------------------------------------------------------------------------------------
// y[p][oy][ox] = sum_ty wy[oy][ty] * ( sum_tx wx[ox][tx] * x[p][iy[oy][ty]][ix[ox][tx]] ),   fp32 [planes][H][W] -> [planes][Ho][Wo]
// The kernel knows no filter: it applies iy / wy [Ho][T] and ix / wx [Wo][T] (int32 / fp32; unused taps: weight 0, valid index).
// A workgroup of four waves owns a TH x TW = 16 x 64 output tile of one plane (grid.z walks the planes):
//   1. stage   the source rows ylo .. ylo + ynum - 1 the tile's row taps name, columns xlo .. xlo + xnum - 1 its column taps
//              name (xlo a multiple of 4), global -> LDS Src[ynum][SW];
//   2. h pass  Hb[r][ox] = sum_tx wx[ox][tx] Src[r][ix[ox][tx] - xlo] for every staged row, LDS -> LDS (lane = output column);
//   3. v pass  y = sum_ty wy[oy][ty] Hb[iy[oy][ty] - ylo][ox], four consecutive columns per lane, 16-byte LDS reads.
// So an output costs Tx + Ty multiply-adds plus its share of the staging, not Tx Ty.  The ranges (ylo, ynum) per tile row and
// (xlo, xnum) per tile column are computed on the host when the plan is made, from the very tables the kernel reads, and a plan
// whose ranges exceed SH x SW is refused there: every LDS index is in range by construction, every global index by the
// plan's check 0 <= idx < n_in.
// Each sum is an fmaf chain in ascending tap order that starts from the first product, and an output is computed from its own
// table rows and source elements alone: its bits do not depend on the tile, the plane's position in the batch, or the path.
// fp32 roundings on an output's longest path, counted as if nothing were fused (as af_sag.hip counts its two passes):
//   h pass  wx_0 v, then Tx - 1 additions        Tx          (the other products are rounded once each, off the path)
//   v pass  wy_0 h, then Ty - 1 additions       +Ty  =>  Tx + Ty
// i.e. |y - exact| <= (Tx + Ty) 2^-24 sum |wy| |wx| |x| to first order; a weight of exactly 1 or 0 rounds nothing, so
// nearest-exact (T = 1, weight 1) is a gather and an identity table returns the input's bits.
// Paths: 16-byte global loads when x is 16-byte aligned and W % 4 == 0 (then every staged group of four columns lies inside its
// row), else element loads; 16-byte stores when y is 16-byte aligned and Wo % 4 == 0, else element stores.  The paths move the
// same values.  Loads before stores; y may not alias x (a tile reads what its neighbours write).
// LDS: Src 32 x 80 + Hb 32 x 64 floats = 18 KiB; registers (46 - 107 by tap count) allow four to eight workgroups per CU.  Hb rows are 256 bytes: the 16 lanes of one output row
// read one whole bank row per 16-byte access.
// ---------------------------------------------------------------------------------------------------------------------------
namespace resample {

enum { TW = 64, TH = 16, SW = 80, SH = 32, kThreads = 256, kMaxTaps = AF_RESAMPLE_MAX_TAPS };

struct Args {
  const float* x;
  float* y;
  const int* iy;
  const float* wy;
  const int* ix;
  const float* wx;
  const int* yr;   // [tiles_y][2]: ylo, ynum
  const int* xr;   // [tiles_x][2]: xlo (a multiple of 4), xnum
  int H, W, Ho, Wo;
  long planes;
};

template <int T, bool VIN, bool VOUT>
__global__ void __launch_bounds__(kThreads) resample_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) float Src[SH * SW];
  __shared__ __attribute__((aligned(16))) float Hb[SH * TW];
  const int tid = threadIdx.x;
  const int ox0 = blockIdx.x * TW, oy0 = blockIdx.y * TH;
  const int ylo = a.yr[2 * blockIdx.y], ynum = a.yr[2 * blockIdx.y + 1];
  const int xlo = a.xr[2 * blockIdx.x], xnum = a.xr[2 * blockIdx.x + 1];
  const int W = a.W, Wo = a.Wo;

  // this lane's column taps (h pass) and row taps (v pass); a lane past the edge takes the last row / column and stores nothing
  const int hx = min(ox0 + (tid & 63), Wo - 1);
  const int q4 = (tid & 15) * 4, vy = oy0 + (tid >> 4), vyc = min(vy, a.Ho - 1);
  int cix[T], ciy[T];
  float cwx[T], cwy[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    cix[t] = a.ix[hx * T + t] - xlo;
    cwx[t] = a.wx[hx * T + t];
    ciy[t] = (a.iy[vyc * T + t] - ylo) * TW + q4;
    cwy[t] = a.wy[vyc * T + t];
  }

  for (long p = blockIdx.z; p < a.planes; p += gridDim.z) {
    const float* xp = a.x + p * a.H * W + (long)ylo * W + xlo;
    if (VIN) {
      const int nv = (xnum + 3) >> 2;
      for (int idx = tid; idx < ynum * nv; idx += kThreads) {
        const int r = idx / nv, v = idx - r * nv;
        *reinterpret_cast<float4*>(&Src[r * SW + 4 * v]) = *reinterpret_cast<const float4*>(xp + (long)r * W + 4 * v);
      }
    } else {
      for (int idx = tid; idx < ynum * xnum; idx += kThreads) {
        const int r = idx / xnum, c = idx - r * xnum;
        Src[r * SW + c] = xp[(long)r * W + c];
      }
    }
    __syncthreads();
    for (int r = tid >> 6; r < ynum; r += kThreads / 64) {
      const float* row = Src + r * SW;
      float s = cwx[0] * row[cix[0]];
#pragma unroll
      for (int t = 1; t < T; ++t) s = fmaf(cwx[t], row[cix[t]], s);
      Hb[r * TW + (tid & 63)] = s;
    }
    __syncthreads();
    if (vy < a.Ho && ox0 + q4 < Wo) {
      float4 v = *reinterpret_cast<const float4*>(&Hb[ciy[0]]);
      float4 s = make_float4(cwy[0] * v.x, cwy[0] * v.y, cwy[0] * v.z, cwy[0] * v.w);
#pragma unroll
      for (int t = 1; t < T; ++t) {
        v = *reinterpret_cast<const float4*>(&Hb[ciy[t]]);
        s.x = fmaf(cwy[t], v.x, s.x);
        s.y = fmaf(cwy[t], v.y, s.y);
        s.z = fmaf(cwy[t], v.z, s.z);
        s.w = fmaf(cwy[t], v.w, s.w);
      }
      float* yp = a.y + (p * a.Ho + vy) * Wo + ox0 + q4;
      if (VOUT) {   // Wo % 4 == 0: a group that starts inside the row ends inside it
        *reinterpret_cast<float4*>(yp) = s;
      } else {
        const int left = Wo - (ox0 + q4);
        yp[0] = s.x;
        if (left > 1) yp[1] = s.y;
        if (left > 2) yp[2] = s.z;
        if (left > 3) yp[3] = s.w;
      }
    }
    // (the next plane's staging writes Src, which nobody reads after the second barrier; its h pass waits at the first)
  }
}

template <int T>
static void launch(bool vin, bool vout, dim3 grid, hipStream_t s, const Args& a) {
  const dim3 block(kThreads);
  if (vin && vout) hipLaunchKernelGGL((resample_kernel<T, true, true>), grid, block, 0, s, a);
  else if (vin) hipLaunchKernelGGL((resample_kernel<T, true, false>), grid, block, 0, s, a);
  else if (vout) hipLaunchKernelGGL((resample_kernel<T, false, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((resample_kernel<T, false, false>), grid, block, 0, s, a);
}

static const int kMaxOut = 8192, kMaxScale = 8;

static const char* mode_name(int mode) {
  switch (mode) {
    case AF_RESAMPLE_NEAREST_EXACT: return "nearest-exact";
    case AF_RESAMPLE_BILINEAR: return "bilinear";
    case AF_RESAMPLE_BICUBIC: return "bicubic";
    case AF_RESAMPLE_LANCZOS3: return "lanczos3";
  }
  return nullptr;
}

static int check_axis(const char* who, int mode, int n_in, int n_out) {
  if (!mode_name(mode)) { af_set_error_msg("%s: unknown mode %d", who, mode); return AF_ERR_INVALID; }
  if (n_in < 1) { af_set_error_msg("%s: n_in = %d: at least one source element expected", who, n_in); return AF_ERR_INVALID; }
  if (n_out < n_in) {
    af_set_error_msg("%s: n_out = %d < n_in = %d: upscaling only (downscaling widens the filter support and is out of scope)", who,
                     n_out, n_in);
    return AF_ERR_INVALID;
  }
  if (n_out > kMaxOut) { af_set_error_msg("%s: n_out = %d exceeds %d", who, n_out, kMaxOut); return AF_ERR_INVALID; }
  if (n_out > kMaxScale * n_in) {
    af_set_error_msg("%s: n_out = %d exceeds %d x n_in = %d", who, n_out, kMaxScale, kMaxScale * n_in);
    return AF_ERR_INVALID;
  }
  return AF_OK;
}

static double sinc(double x) {
  if (x == 0.0) return 1.0;
  x *= M_PI;
  return std::sin(x) / x;
}

}  // namespace resample

struct af_resample_plan {
  int mode, H, W, Ho, Wo, T, tiles_y, tiles_x, device;
  std::vector<int32_t> iy, ix, yr, xr;
  std::vector<float> wy, wx;
  char* dev;   // one allocation: iy | ix | yr | xr | wy | wx
  resample::Args args;
};

extern "C" {

int64_t af_resample2d_launches(void) { return (int64_t)g_af_resample2d_launches.load(std::memory_order_relaxed); }

int af_resample_taps(int mode, int n_in, int n_out, int32_t* idx, double* w, int* taps) {
  // The only place of the product that states the filters.  Row o of idx / w holds output o's taps, [n_out][*taps].
  using namespace resample;
  if (!idx || !w || !taps) { af_set_error_msg("af_resample_taps: null argument"); return AF_ERR_INVALID; }
  if (int rc = check_axis("af_resample_taps", mode, n_in, n_out)) return rc;
  const int last = n_in - 1;
  auto clampi = [last](long i) { return (int32_t)(i < 0 ? 0 : (i > last ? last : i)); };
  if (mode == AF_RESAMPLE_NEAREST_EXACT) {
    *taps = 1;
    for (int o = 0; o < n_out; ++o) {
      idx[o] = clampi((long)std::floor((o + 0.5) * n_in / n_out));
      w[o] = 1.0;
    }
    return AF_OK;
  }
  const double s = (double)n_in / (double)n_out;
  if (mode == AF_RESAMPLE_BILINEAR) {   // torch: the source coordinate is clamped at 0, the upper index at the edge
    *taps = 2;
    for (int o = 0; o < n_out; ++o) {
      double c = (o + 0.5) * s - 0.5;
      if (c < 0.0) c = 0.0;
      const long i0 = (long)std::floor(c);
      const double l1 = c - (double)i0;
      idx[2 * o] = clampi(i0);
      idx[2 * o + 1] = clampi(i0 + 1);
      w[2 * o] = 1.0 - l1;
      w[2 * o + 1] = l1;
    }
    return AF_OK;
  }
  if (mode == AF_RESAMPLE_BICUBIC) {   // torch: cubic convolution with A = -0.75, the coordinate unclamped, the indices clamped
    *taps = 4;
    const double A = -0.75;
    auto c1 = [A](double x) { return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0; };
    auto c2 = [A](double x) { return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A; };
    for (int o = 0; o < n_out; ++o) {
      const double c = (o + 0.5) * s - 0.5;
      const double fl = std::floor(c);
      const long i0 = (long)fl;
      const double t = c - fl;
      for (int k = 0; k < 4; ++k) idx[4 * o + k] = clampi(i0 - 1 + k);
      w[4 * o] = c2(t + 1.0);
      w[4 * o + 1] = c1(t);
      w[4 * o + 2] = c1(1.0 - t);
      w[4 * o + 3] = c2((1.0 - t) + 1.0);
    }
    return AF_OK;
  }
  // lanczos3, Pillow's precompute_coeffs for upscaling (filter scale 1): window [int(c - 3 + 0.5), int(c + 3 + 0.5)) cut to the
  // axis, weights lanczos(x + xmin - c + 0.5) renormalised over the window; the taps left over repeat the last index at weight 0
  *taps = 7;
  for (int o = 0; o < n_out; ++o) {
    const double c = (o + 0.5) * s;
    int xmin = (int)(c - 3.0 + 0.5), xmax = (int)(c + 3.0 + 0.5);
    if (xmin < 0) xmin = 0;
    if (xmax > n_in) xmax = n_in;
    int n = xmax - xmin;
    if (n > 7) n = 7;
    double sum = 0.0;
    for (int k = 0; k < n; ++k) {
      const double x = (double)(k + xmin) - c + 0.5;
      const double v = (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3.0) : 0.0;
      w[7 * o + k] = v;
      sum += v;
    }
    for (int k = 0; k < 7; ++k) {
      idx[7 * o + k] = clampi(xmin + (k < n ? k : n - 1));
      w[7 * o + k] = k < n && sum != 0.0 ? w[7 * o + k] / sum : 0.0;
    }
  }
  return AF_OK;
}

int af_resample_plan_create(int mode, int H, int W, int Ho, int Wo, af_resample_plan** plan) {
  using namespace resample;
  if (!plan) { af_set_error_msg("af_resample_plan_create: null plan pointer"); return AF_ERR_INVALID; }
  *plan = nullptr;
  if (int rc = check_axis("af_resample_plan_create (rows)", mode, H, Ho)) return rc;
  if (int rc = check_axis("af_resample_plan_create (columns)", mode, W, Wo)) return rc;
  af_resample_plan* P = new af_resample_plan();
  P->mode = mode; P->H = H; P->W = W; P->Ho = Ho; P->Wo = Wo; P->dev = nullptr;
  auto fail = [&](int rc) { delete P; return rc; };
  // both axes' tables: weights rounded to fp32 once, here; every entry checked before anything reaches the device
  auto axis = [&](const char* name, int n_in, int n_out, std::vector<int32_t>& iv, std::vector<float>& wv, int& T) -> int {
    std::vector<int32_t> i64((size_t)n_out * kMaxTaps);
    std::vector<double> wd((size_t)n_out * kMaxTaps);
    if (int rc = af_resample_taps(mode, n_in, n_out, i64.data(), wd.data(), &T)) return rc;
    iv.assign(i64.begin(), i64.begin() + (size_t)n_out * T);
    wv.resize((size_t)n_out * T);
    for (size_t k = 0; k < wv.size(); ++k) {
      wv[k] = (float)wd[k];
      if (iv[k] < 0 || iv[k] >= n_in || !std::isfinite(wv[k])) {
        af_set_error_msg("af_resample_plan_create: %s table entry %zu (index %d, weight %g) outside [0, %d) / not finite", name, k,
                         (int)iv[k], wd[k], n_in);
        return AF_ERR_INVALID;
      }
    }
    return AF_OK;
  };
  int Ty = 0, Tx = 0;
  if (int rc = axis("row", H, Ho, P->iy, P->wy, Ty)) return fail(rc);
  if (int rc = axis("column", W, Wo, P->ix, P->wx, Tx)) return fail(rc);
  if (Ty != Tx || (Tx != 1 && Tx != 2 && Tx != 4 && Tx != 7)) {
    af_set_error_msg("af_resample_plan_create: %d x %d taps have no kernel instance", Ty, Tx);
    return fail(AF_ERR_INVALID);
  }
  P->T = Tx;
  // per tile row / column: the source range its taps name; what does not fit the kernel's LDS image is refused here
  auto ranges = [&](const char* name, const std::vector<int32_t>& iv, int n_out, int tile, int cap, int align, std::vector<int32_t>& out,
                    int& tiles) -> int {
    tiles = (n_out + tile - 1) / tile;
    out.resize((size_t)2 * tiles);
    for (int b = 0; b < tiles; ++b) {
      int lo = iv[(size_t)b * tile * P->T], hi = lo;
      const int end = std::min(n_out, (b + 1) * tile);
      for (size_t k = (size_t)b * tile * P->T; k < (size_t)end * P->T; ++k) { lo = std::min(lo, (int)iv[k]); hi = std::max(hi, (int)iv[k]); }
      lo -= lo % align;
      const int num = hi - lo + 1;
      if ((num + align - 1) / align * align > cap) {
        af_set_error_msg("af_resample_plan_create: %s tile %d needs %d source elements, the kernel stages %d", name, b, num, cap);
        return AF_ERR_INVALID;
      }
      out[2 * b] = lo;
      out[2 * b + 1] = num;
    }
    return AF_OK;
  };
  if (int rc = ranges("row", P->iy, Ho, TH, SH, 1, P->yr, P->tiles_y)) return fail(rc);
  if (int rc = ranges("column", P->ix, Wo, TW, SW, 4, P->xr, P->tiles_x)) return fail(rc);

  const std::vector<int32_t>* ivs[4] = {&P->iy, &P->ix, &P->yr, &P->xr};
  const std::vector<float>* wvs[2] = {&P->wy, &P->wx};
  size_t off[6], bytes = 0;
  for (int k = 0; k < 6; ++k) {
    off[k] = bytes;
    const size_t n = k < 4 ? ivs[k]->size() : wvs[k - 4]->size();
    bytes += (n * 4 + 15) / 16 * 16;
  }
  if (hipGetDevice(&P->device) != hipSuccess) { af_set_error_msg("af_resample_plan_create: no HIP device"); return fail(AF_ERR_HIP); }
  hipError_t e = hipMalloc((void**)&P->dev, bytes);
  for (int k = 0; k < 6 && e == hipSuccess; ++k) {
    const void* src = k < 4 ? (const void*)ivs[k]->data() : (const void*)wvs[k - 4]->data();
    const size_t n = k < 4 ? ivs[k]->size() : wvs[k - 4]->size();
    e = hipMemcpy(P->dev + off[k], src, n * 4, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    af_set_error_msg("af_resample_plan_create: device tables: %s", hipGetErrorString(e));
    if (P->dev) (void)hipFree(P->dev);
    return fail(AF_ERR_HIP);
  }
  P->args = Args{nullptr, nullptr, (const int*)(P->dev + off[0]), (const float*)(P->dev + off[4]), (const int*)(P->dev + off[1]),
                 (const float*)(P->dev + off[5]), (const int*)(P->dev + off[2]), (const int*)(P->dev + off[3]), H, W, Ho, Wo, 0};
  *plan = P;
  return AF_OK;
}

int af_resample_plan_destroy(af_resample_plan* plan) {
  if (!plan) return AF_OK;
  if (plan->dev) (void)hipFree(plan->dev);
  delete plan;
  return AF_OK;
}

int af_resample_plan_tables(const af_resample_plan* plan, int* taps, int32_t* iy, float* wy, int32_t* ix, float* wx) {
  if (!plan || !taps) { af_set_error_msg("af_resample_plan_tables: null argument"); return AF_ERR_INVALID; }
  *taps = plan->T;
  if (iy) std::copy(plan->iy.begin(), plan->iy.end(), iy);
  if (wy) std::copy(plan->wy.begin(), plan->wy.end(), wy);
  if (ix) std::copy(plan->ix.begin(), plan->ix.end(), ix);
  if (wx) std::copy(plan->wx.begin(), plan->wx.end(), wx);
  return AF_OK;
}

int af_resample2d(const af_resample_plan* plan, const float* x_dev, float* y_dev, int64_t planes, void* stream) {
  using namespace resample;
  if (!plan || !x_dev || !y_dev) { af_set_error_msg("af_resample2d: null argument"); return AF_ERR_INVALID; }
  const long nin = (long)plan->H * plan->W, nout = (long)plan->Ho * plan->Wo;
  if (planes <= 0 || planes > (1L << 40) / nout) {
    af_set_error_msg("af_resample2d: %lld planes of %d x %d outputs", (long long)planes, plan->Ho, plan->Wo);
    return AF_ERR_INVALID;
  }
  if ((uintptr_t)x_dev < (uintptr_t)(y_dev + planes * nout) && (uintptr_t)y_dev < (uintptr_t)(x_dev + planes * nin)) {
    af_set_error_msg("af_resample2d: the output must not alias the input (a tile reads what its neighbours write)");
    return AF_ERR_INVALID;
  }
  Args a = plan->args;
  a.x = x_dev;
  a.y = y_dev;
  a.planes = (long)planes;
  const bool vin = ((uintptr_t)x_dev & 15) == 0 && plan->W % 4 == 0;
  const bool vout = ((uintptr_t)y_dev & 15) == 0 && plan->Wo % 4 == 0;
  const dim3 grid((unsigned)plan->tiles_x, (unsigned)plan->tiles_y, (unsigned)std::min<long>(planes, 65535));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch (plan->T) {
    case 1: launch<1>(vin, vout, grid, s, a); break;
    case 2: launch<2>(vin, vout, grid, s, a); break;
    case 4: launch<4>(vin, vout, grid, s, a); break;
    default: launch<7>(vin, vout, grid, s, a); break;
  }
  HIP_CHECK_RET(hipGetLastError());
  g_af_resample2d_launches.fetch_add(1, std::memory_order_relaxed);
  return AF_OK;
}

}  // extern "C"
