// Operator-level C-ABI entry points used by the parity tests (tests/test_ops_gpu.py).
// They take fp32 device tensors in the REFERENCE's layouts (NCHW, [rows, C],
// [B, N, heads*dh]), convert to the internal NHWC storage dtype, run exactly the
// kernels the UNet / VAE executors use, and convert back.  Temporary buffers are
// hipMalloc'd per call (test path only, never on the hot path).
#include "../../include/adaface_hip.h"
#include "af_host.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {
struct Tmp {
  std::vector<void*> bufs;
  void* get(size_t bytes, bool zero = false) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nullptr;
    if (zero) hipMemset(p, 0, bytes);
    bufs.push_back(p);
    return p;
  }
  ~Tmp() {
    hipDeviceSynchronize();
    for (void* p : bufs) hipFree(p);
  }
};
}  // namespace

// columns [c0, ld) of every row of a [rows][ld] buffer of T become v (slack columns of a wide-row test buffer; c0 = 0: the whole buffer)
template <typename T> __global__ __launch_bounds__(256) void fill_cols_kernel(T* __restrict__ y, long rows, int ld, int c0, float v) {
  const int w = ld - c0;
  const long n = rows * w;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / w;
    y[r * ld + c0 + (int)(i - r * w)] = from_f32<T>(v);
  }
}
template <typename T> static int fill_cols(void* y, long rows, int ld, int c0, float v, hipStream_t s) {
  const long n = rows * (ld - c0);
  if (n <= 0) return 0;
  const long nb = (n + 255) / 256;
  hipLaunchKernelGGL((fill_cols_kernel<T>), dim3((unsigned)(nb > 4096 ? 4096 : nb)), dim3(256), 0, s, reinterpret_cast<T*>(y), rows, ld, c0, v);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
static int fill_cols_dt(int dtype, void* y, long rows, int ld, int c0, float v, hipStream_t s) {
  return AF_TYPED(dtype, fill_cols<Elem>(y, rows, ld, c0, v, s));
}
// what af_op_conv2d_ex / af_op_linear_ex put into the output buffer before the launch (exact in bf16 / fp16, above any result of
// the tests) and into the slack columns of the operands
static const float OP_SENTINEL = 49152.f;   // 3 * 2^14
static const float OP_NAN = __builtin_nanf("");

#define OP_ALLOC(var, bytes, zero)                               \
  void* var = tmp.get((bytes), (zero));                          \
  if (!var) { af_set_error_msg("hipMalloc failed in op"); return AF_ERR_HIP; }

// ---- device clock probe (bench.py --full stamps its line with it: devices of one pool hold different clocks under MFMA load, so
// whole-path numbers from different boxes are only comparable through a number like this) ----
// Every wave runs `iters` rounds of four independent v_mfma_f32_32x32x16_bf16 on pseudo-random register operands (no memory
// traffic, no LDS) between two (s_memtime, s_memrealtime) stamp pairs: shader cycles / 100 MHz reference ticks = the clock
// the chip holds under a dense MFMA stream.  The stamps go to a buffer nothing else reads; the accumulators to a sink.
__global__ __launch_bounds__(256) void clock_probe_kernel(unsigned long long* __restrict__ stamps, float* __restrict__ sink,
                                                          int iters) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned hsh = (blockIdx.x * 256u + threadIdx.x) * 2654435761u + 12345u;
  bf16x8 a, b;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    hsh = hsh * 1664525u + 1013904223u;
    a[e] = (bf16)(((int)(hsh >> 16) & 0xFF) * (1.0f / 128.0f) - 1.0f);
    hsh = hsh * 1664525u + 1013904223u;
    b[e] = (bf16)(((int)(hsh >> 16) & 0xFF) * (1.0f / 128.0f) - 1.0f);
  }
  f32x16 c0, c1, c2, c3;
#pragma unroll
  for (int r = 0; r < 16; ++r) { c0[r] = 0.f; c1[r] = 0.f; c2[r] = 0.f; c3[r] = 0.f; }
  const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  for (int i = 0; i < iters; ++i) {
    c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b, a, c1, 0, 0, 0);
    c2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, a, c2, 0, 0, 0);
    c3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b, b, c3, 0, 0, 0);
  }
  asm volatile("" : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3));
  const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  if (lane == 0) {
    stamps[((size_t)blockIdx.x * 4 + wave) * 2 + 0] = t1 - t0;
    stamps[((size_t)blockIdx.x * 4 + wave) * 2 + 1] = r1 - r0;
  }
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc += c0[r] + c1[r] + c2[r] + c3[r];
  sink[blockIdx.x * 256 + threadIdx.x] = acc;
}

extern "C" {

int af_clock_probe(void* stream, int iters, double* mfma_mhz, double* mfma_tflops) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (iters <= 0) iters = 40000;
  hipDeviceProp_t prop;
  int dev = 0;
  HIP_CHECK_RET(hipGetDevice(&dev));
  HIP_CHECK_RET(hipGetDeviceProperties(&prop, dev));
  const int blocks = 2 * prop.multiProcessorCount;    // two waves per SIMD: every matrix pipe is kept busy
  Tmp tmp;
  OP_ALLOC(stamps, (size_t)blocks * 4 * 2 * sizeof(unsigned long long), true);
  OP_ALLOC(sink, (size_t)blocks * 256 * sizeof(float), false);
  struct Ev {   // destroyed on every exit path
    hipEvent_t e = nullptr;
    ~Ev() { if (e) hipEventDestroy(e); }
  } ev0, ev1;
  HIP_CHECK_RET(hipEventCreate(&ev0.e));
  HIP_CHECK_RET(hipEventCreate(&ev1.e));
  hipEvent_t e0 = ev0.e, e1 = ev1.e;
  // one short launch to wake the device, then the timed one
  hipLaunchKernelGGL(clock_probe_kernel, dim3(blocks), dim3(256), 0, s, (unsigned long long*)stamps, (float*)sink, 2000);
  HIP_CHECK_RET(hipEventRecord(e0, s));
  hipLaunchKernelGGL(clock_probe_kernel, dim3(blocks), dim3(256), 0, s, (unsigned long long*)stamps, (float*)sink, iters);
  HIP_CHECK_RET(hipEventRecord(e1, s));
  HIP_CHECK_RET(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_CHECK_RET(hipEventElapsedTime(&ms, e0, e1));
  std::vector<unsigned long long> h((size_t)blocks * 8);
  HIP_CHECK_RET(hipMemcpy(h.data(), stamps, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  std::vector<double> mhz;
  for (size_t i = 0; i < h.size(); i += 2)
    if (h[i + 1] > 0) mhz.push_back((double)h[i] / (double)h[i + 1] * 100.0);
  if (mhz.empty()) { af_set_error_msg("af_clock_probe: no stamps"); return AF_ERR_STATE; }
  std::sort(mhz.begin(), mhz.end());
  if (mfma_mhz) *mfma_mhz = mhz[mhz.size() / 2];
  if (mfma_tflops) *mfma_tflops = (double)blocks * 4 * (double)iters * 4 * (2.0 * 32 * 32 * 16) / (ms * 1e-3) / 1e12;
  return AF_OK;
}

// af_op_conv2d with the launch forms only the model states (Runner::conv_params, af_model.hip): a per-sample bias row
// (rowbias_dev: float [B][Cout], cast to the storage type), alpha on the accumulator, the VAE encoder's bottom / right-only
// padding (pad 0: 3x3, stride 2, even maps; pad -1: ks / 2) and row pitches wider than the channel count (ld_slack elements,
// a multiple of 8, added to ldc / ldo / ldr / ldrb).  The slack of the source, the residual and the bias row holds NaN, the
// whole output buffer the sentinel before the launch.  ld_slack > 0: y_dev receives the whole rows, float [B * Ho * Wo][ldo]
// with ldo = round_up(Cout, 4) + ld_slack; otherwise NCHW as af_op_conv2d.
int af_op_conv2d_ex(int dtype, const float* x_dev, const float* w_dev, const float* bias_dev, const float* residual_dev,
                    const float* rowbias_dev, float alpha, float* y_dev, int B, int Cin, int H, int W, int Cout, int ks, int stride,
                    int pad, int upsample, int ld_slack, void* stream) {
  if (pad < 0) pad = ks / 2;
  const bool br_pad = pad == 0 && ks == 3 && stride == 2 && !upsample && H % 2 == 0 && W % 2 == 0;   // bottom / right only
  if ((ks != 1 && ks != 3) || (pad != ks / 2 && !br_pad)) {
    af_set_error_msg("af_op_conv2d_ex: ks must be 1 or 3 with pad ks/2 (pad 0: 3x3, stride 2, even maps, no upsampling)");
    return AF_ERR_INVALID;
  }
  if (ld_slack < 0 || ld_slack % 8 != 0) { af_set_error_msg("af_op_conv2d_ex: ld_slack must be a non-negative multiple of 8"); return AF_ERR_INVALID; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  const int cin_pad = round_up(Cin, bk_of(dtype));
  const int Hi = H << upsample, Wi = W << upsample;
  // (pad 0: one row / column of zeros below and to the right, as the model's (H + 1 - 3) / 2 + 1)
  const int Ho = br_pad ? (Hi + 1 - ks) / stride + 1 : (Hi + 2 * pad - ks) / stride + 1;
  const int Wo = br_pad ? (Wi + 1 - ks) / stride + 1 : (Wi + 2 * pad - ks) / stride + 1;
  const int co4 = round_up(Cout, 4), rows_pad = round_up(Cout, 128), ldw = ks * ks * cin_pad;
  const int ldc = cin_pad + ld_slack, ldo = co4 + ld_slack;
  const long M = (long)B * Ho * Wo;
  OP_ALLOC(xn, (size_t)B * H * W * ldc * esize(dtype), false);
  OP_ALLOC(wn, (size_t)rows_pad * ldw * esize(dtype), true);
  OP_ALLOC(yn, (size_t)M * ldo * esize(dtype), false);
  void* rn = nullptr;
  void* rbn = nullptr;
  float* bn = nullptr;
  AF_TRY(fill_cols_dt(dtype, yn, M, ldo, 0, OP_SENTINEL, s));
  AF_TRY(AF_TYPED(dtype, af_launch_nchw_to_nhwc<Elem>(x_dev, xn, B, Cin, H * W, ldc, 1.f, s)));
  AF_TRY(fill_cols_dt(dtype, xn, (long)B * H * W, ldc, cin_pad, OP_NAN, s));
  AF_TRY(AF_TYPED(dtype, af_launch_repack_weight<Elem>(w_dev, wn, Cout, Cin, cin_pad, ks, ldw, 0, 0, s)));
  if (bias_dev) {
    bn = reinterpret_cast<float*>(tmp.get((size_t)round_up(Cout, 128) * 4, true));
    if (!bn) return AF_ERR_HIP;
    if (hipMemcpyAsync(bn, bias_dev, (size_t)Cout * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return AF_ERR_HIP;
  }
  if (residual_dev) {
    rn = tmp.get((size_t)M * ldo * esize(dtype), false);
    if (!rn) return AF_ERR_HIP;
    AF_TRY(AF_TYPED(dtype, af_launch_nchw_to_nhwc<Elem>(residual_dev, rn, B, Cout, Ho * Wo, ldo, 1.f, s)));
    AF_TRY(fill_cols_dt(dtype, rn, M, ldo, co4, OP_NAN, s));
  }
  if (rowbias_dev) {   // [B][Cout] rows = NCHW with one pixel per sample
    rbn = tmp.get((size_t)B * ldo * esize(dtype), false);
    if (!rbn) return AF_ERR_HIP;
    AF_TRY(AF_TYPED(dtype, af_launch_nchw_to_nhwc<Elem>(rowbias_dev, rbn, B, Cout, 1, ldo, 1.f, s)));
    AF_TRY(fill_cols_dt(dtype, rbn, B, ldo, co4, OP_NAN, s));
  }
  ConvGemmParams p;
  memset(&p, 0, sizeof(p));
  p.src = xn; p.src_batch_stride = (long)H * W * ldc; p.ldc = ldc; p.Cin = cin_pad;
  p.Hs = H; p.Ws = W; p.up = upsample; p.Hi = Hi; p.Wi = Wi; p.Ho = Ho; p.Wo = Wo;
  p.ks = ks; p.stride = stride; p.pad = pad;
  p.W = wn; p.ldw = ldw; p.Wrows = rows_pad;
  p.M = (int)M; p.N = co4; p.K = ldw;
  p.bias = bn; p.residual = rn; p.ldr = ldo; p.out = yn; p.ldo = ldo; p.alpha = alpha;
  p.rowbias = rbn; p.ldrb = ldo;
  p.k_logical = ks * ks * Cin;
  if (upsample && ks == 3 && dtype == AF_DTYPE_BF16 && cin_pad % 64 == 0) {
    // as the model does for its Upsample layers: phase weights next to the 3x3 ones, the launcher decides (AF_CONV_UP_PHASE4)
    OP_ALLOC(w4, (size_t)4 * rows_pad * 4 * cin_pad * 2, false);
    AF_TRY(af_launch_up_phase4_weights(wn, rows_pad, cin_pad, ldw, w4, s));
    p.W_up4 = w4;
  }
  const AfGemmPlan pl = af_plan_conv_gemm(p, 1, storage_of(dtype));
  void* ws = nullptr;
  if (pl.splitk > 1) { ws = tmp.get(pl.ws_bytes, false); if (!ws) return AF_ERR_HIP; }
  AF_TRY(AF_TYPED(dtype, af_launch_conv_gemm<Elem>(p, 1, s, &pl, ws)));
  if (ld_slack > 0) {
    AF_TRY(AF_TYPED(dtype, af_launch_cast_to_f32<Elem>(yn, y_dev, M * ldo, s)));
    return 0;
  }
  AF_TRY(AF_TYPED(dtype, af_launch_nhwc_to_nchw<Elem>(yn, y_dev, B, Cout, Ho * Wo, co4, s)));
  return 0;
}
int af_op_conv2d(int dtype, const float* x_dev, const float* w_dev, const float* bias_dev, const float* residual_dev,
                 float* y_dev, int B, int Cin, int H, int W, int Cout, int ks, int stride, int pad, int upsample,
                 void* stream) {
  if ((ks != 1 && ks != 3) || pad != ks / 2) { af_set_error_msg("af_op_conv2d: ks must be 1 or 3 with pad ks/2"); return AF_ERR_INVALID; }
  return af_op_conv2d_ex(dtype, x_dev, w_dev, bias_dev, residual_dev, nullptr, 1.f, y_dev, B, Cin, H, W, Cout, ks, stride, pad, upsample, 0, stream);
}

// Host-only diagnostic: the plan af_launch_conv_gemm would follow for a launch described by integers.  Parameters as af_op_conv2d
// / af_op_linear build them (a linear: ks 1, the M rows as one 1 x M map), flagged operands as aligned dummies, alpha 1; no device
// is touched.  out7 = {kernel (AfGemmKernel), row-panel kind, tile, splitk, halo_tw, group_m, ws_bytes}
int af_gemm_plan_query(int dtype, int64_t M, int N, int K, int cin_pad, int ks, int stride, int pad, int up, int Hs, int Ws, int Ho,
                       int Wo, int ldc, int ldo, int gn_hw, int gn_cpg, int flags, int64_t* out7) {
  if (!out7 || M <= 0 || M > 0x7fffffff || (dtype != AF_DTYPE_BF16 && dtype != AF_DTYPE_F32 && dtype != AF_DTYPE_F16)) {
    af_set_error_msg("af_gemm_plan_query: bad argument");
    return AF_ERR_INVALID;
  }
  alignas(16) static char dummy[16];
  void* const d = dummy;
  ConvGemmParams p;
  memset(&p, 0, sizeof(p));
  p.src = d; p.src_batch_stride = (long)Hs * Ws * ldc; p.ldc = ldc; p.Cin = cin_pad;
  p.Hs = Hs; p.Ws = Ws; p.up = up; p.Hi = Hs << up; p.Wi = Ws << up; p.Ho = Ho; p.Wo = Wo;
  p.ks = ks; p.stride = stride; p.pad = pad;
  p.W = d; p.ldw = K; p.Wrows = round_up(N, 128);
  p.M = (int)M; p.N = N; p.K = K; p.k_logical = K;
  p.out = d; p.ldo = ldo; p.alpha = 1.f;
  if (flags & AF_PQ_GEGLU) p.epilogue = AF_EPI_GEGLU;
  if (flags & AF_PQ_RESIDUAL) { p.residual = d; p.ldr = ldo; }
  if (flags & AF_PQ_ROWBIAS) { p.rowbias = d; p.ldrb = N; }
  if (flags & AF_PQ_LN_CONSUMER) { p.ln_stats = reinterpret_cast<const float*>(d); p.ln_colsum = reinterpret_cast<const float*>(d); }
  if (flags & AF_PQ_LN_PRODUCER) p.ln_stats_out = reinterpret_cast<float*>(d);
  if (flags & AF_PQ_GN_AB) { p.gn_ab = reinterpret_cast<const float*>(d); p.gn_hw = gn_hw; }
  if (flags & AF_PQ_GN_STATS_OUT) { p.gn_stats_out = reinterpret_cast<float*>(d); p.gn_cpg = gn_cpg; }
  if (flags & AF_PQ_FP8) { p.fp8 = 1; p.w_scale = reinterpret_cast<const unsigned char*>(d); p.x_scale_e8 = 127; }
  if (flags & AF_PQ_PHASE_WEIGHTS) p.W_up4 = d;
  const AfGemmPlan pl = af_plan_conv_gemm(p, 1, storage_of(dtype), (flags & AF_PQ_WORKSPACE) != 0);
  const int64_t o[7] = {pl.kernel, pl.rowpanel, pl.tile, pl.splitk, pl.halo_tw, pl.group_m, (int64_t)pl.ws_bytes};
  memcpy(out7, o, sizeof(o));
  return AF_OK;
}

// Host-only diagnostic: the plan af_launch_groupnorm (kind 0) or af_launch_layernorm (kind 1) would follow; no device is
// touched.  kind 0: n = pixels per sample, out5 = {kernel (AfGnKernel), P, nchunk, npart, wide_stats}; kind 1: n = rows (B and
// pre_npart unused), out5 = {kernel (AfLnKernel), vectors per lane, rows per block, 0, 0}
int af_norm_plan_query(int kind, int dtype, int B, int64_t n, int C, int pre_npart, int64_t* out5) {
  if (!out5 || (kind != 0 && kind != 1) || n < 0 || (kind == 0 && n > 0x7fffffff) ||
      (dtype != AF_DTYPE_BF16 && dtype != AF_DTYPE_F32 && dtype != AF_DTYPE_F16)) {
    af_set_error_msg("af_norm_plan_query: bad argument");
    return AF_ERR_INVALID;
  }
  if (kind == 0) {
    const AfGnPlan pl = af_plan_groupnorm(storage_of(dtype), B, (int)n, C, pre_npart);
    const int64_t o[5] = {pl.kernel, pl.P, pl.nchunk, pl.npart, pl.wide_stats};
    memcpy(out5, o, sizeof(o));
  } else {
    const AfLnPlan pl = af_plan_layernorm(storage_of(dtype), (long)n, C);
    const int64_t o[5] = {pl.kernel, pl.nv, pl.rows_per_block, 0, 0};
    memcpy(out5, o, sizeof(o));
  }
  return AF_OK;
}

// activation shifts of the fp8 mode: e4m3 of value * 2^s, s in [AF_FP8_SHIFT_MIN, AF_FP8_SHIFT_MAX] (adaface_hip.h)
static bool act_shift_ok(int act_shift, const char* who) {
  if (act_shift >= AF_FP8_SHIFT_MIN && act_shift <= AF_FP8_SHIFT_MAX) return true;
  af_set_error_msg("%s: act_shift %d outside [%d, %d]", who, act_shift, AF_FP8_SHIFT_MIN, AF_FP8_SHIFT_MAX);
  return false;
}

// fp8 convolution as the UNet's fp8 mode runs it (bf16 storage): x is cast to bf16, multiplied by 2^act_shift and stored
// as e4m3 (what the GroupNorm kernels write), the weight is repacked to bf16 and quantised per output row
// (af_launch_quant_weight_fp8), the ping-pong kernel multiplies on the block-scaled fp8 MFMA; bias / residual / output bf16.
// Returns AF_ERR_INVALID when the shape has no fp8 plan (the model keeps such layers on bf16).
int af_op_conv2d_fp8(const float* x_dev, const float* w_dev, const float* bias_dev, const float* residual_dev, float* y_dev,
                     int B, int Cin, int H, int W, int Cout, int ks, int stride, int pad, int upsample, int act_shift,
                     void* stream) {
  if ((ks != 1 && ks != 3) || pad != ks / 2 || Cin % 64 != 0) { af_set_error_msg("af_op_conv2d_fp8: ks 1|3, pad ks/2, Cin%%64==0"); return AF_ERR_INVALID; }
  if (!act_shift_ok(act_shift, "af_op_conv2d_fp8")) return AF_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  const int Hi = H << upsample, Wi = W << upsample;
  const int Ho = (Hi + 2 * pad - ks) / stride + 1, Wo = (Wi + 2 * pad - ks) / stride + 1;
  const int co4 = round_up(Cout, 4), rows_pad = round_up(Cout, 128), ldw = ks * ks * Cin, k8 = round_up(ldw, 128);
  const size_t nx = (size_t)B * H * W * Cin;
  OP_ALLOC(xn, nx * 2, false);
  OP_ALLOC(x8, nx, false);
  OP_ALLOC(wn, (size_t)rows_pad * ldw * 2, true);
  OP_ALLOC(w8, (size_t)rows_pad * k8 + rows_pad, true);
  OP_ALLOC(yn, (size_t)B * Ho * Wo * co4 * 2, true);
  unsigned char* sc = reinterpret_cast<unsigned char*>(w8) + (size_t)rows_pad * k8;
  void* rn = nullptr;
  float* bn = nullptr;
  AF_TRY(af_launch_nchw_to_nhwc<bf16>(x_dev, xn, B, Cin, H * W, Cin, 1.f, s));
  AF_TRY(af_launch_cast_fp8(xn, x8, (long)nx, ldexpf(1.f, act_shift), s));
  AF_TRY(af_launch_repack_weight<bf16>(w_dev, wn, Cout, Cin, Cin, ks, ldw, 0, 0, s));
  AF_TRY(af_launch_quant_weight_fp8(wn, rows_pad, ldw, Cin, ks, w8, k8, sc, s));
  if (bias_dev) {
    bn = reinterpret_cast<float*>(tmp.get((size_t)rows_pad * 4, true));
    if (!bn) return AF_ERR_HIP;
    if (hipMemcpyAsync(bn, bias_dev, (size_t)Cout * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return AF_ERR_HIP;
  }
  if (residual_dev) {
    rn = tmp.get((size_t)B * Ho * Wo * co4 * 2, false);
    if (!rn) return AF_ERR_HIP;
    AF_TRY(af_launch_nchw_to_nhwc<bf16>(residual_dev, rn, B, Cout, Ho * Wo, co4, 1.f, s));
  }
  ConvGemmParams p;
  memset(&p, 0, sizeof(p));
  p.src = x8; p.src_batch_stride = (long)H * W * Cin; p.ldc = Cin; p.Cin = Cin;
  p.Hs = H; p.Ws = W; p.up = upsample; p.Hi = Hi; p.Wi = Wi; p.Ho = Ho; p.Wo = Wo;
  p.ks = ks; p.stride = stride; p.pad = pad;
  p.W = w8; p.ldw = k8; p.Wrows = rows_pad;
  p.M = B * Ho * Wo; p.N = co4; p.K = k8;
  p.bias = bn; p.residual = rn; p.ldr = co4; p.out = yn; p.ldo = co4; p.alpha = 1.f;
  p.k_logical = ks * ks * Cin;
  p.fp8 = 1; p.w_scale = sc; p.x_scale_e8 = 127 - act_shift;
  const AfGemmPlan pl = af_plan_conv_gemm(p, 1, AF_ST_BF16);
  if (pl.kernel != AF_GK_PP_FP8) { af_set_error_msg("af_op_conv2d_fp8: no fp8 plan for M=%d N=%d K=%d", p.M, p.N, p.K); return AF_ERR_INVALID; }
  void* ws = nullptr;
  if (pl.splitk > 1) { ws = tmp.get(pl.ws_bytes, false); if (!ws) return AF_ERR_HIP; }
  AF_TRY(af_launch_conv_gemm<bf16>(p, 1, s, &pl, ws));
  AF_TRY(af_launch_nhwc_to_nchw<bf16>(yn, y_dev, B, Cout, Ho * Wo, co4, s));
  return 0;
}

// GroupNorm (+SiLU) with the e4m3 output the fp8 convolutions read: y8_dev [B][H*W][C] bytes of result * 2^act_shift
// rec_out_dev (af_op_groupnorm_fp8_rec): two 32-bit words, {max |result| as a float, number of elements with |result * 2^act_shift| > 448}
static int op_groupnorm_fp8(const float* x_dev, const float* gamma_dev, const float* beta_dev, float eps, int silu,
                            unsigned char* y8_dev, int B, int C, int H, int W, int act_shift, unsigned* rec_out_dev, void* stream) {
  if (!act_shift_ok(act_shift, "af_op_groupnorm_fp8")) return AF_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  const int HW = H * W;
  OP_ALLOC(xn, (size_t)B * HW * C * 2, false);
  OP_ALLOC(ws, af_gn_workspace_bytes(B, HW), false);
  if (rec_out_dev && hipMemsetAsync(rec_out_dev, 0, 2 * sizeof(unsigned), s) != hipSuccess) return AF_ERR_HIP;
  AF_TRY(af_launch_nchw_to_nhwc<bf16>(x_dev, xn, B, C, HW, C, 1.f, s));
  AF_TRY(af_launch_groupnorm<bf16>(xn, (long)HW * C, C, B, HW, C, gamma_dev, beta_dev, eps, silu, y8_dev, (long)HW * C, C, ws, s,
                                   ldexpf(1.f, act_shift), nullptr, 0, rec_out_dev));
  return 0;
}
int af_op_groupnorm_fp8(const float* x_dev, const float* gamma_dev, const float* beta_dev, float eps, int silu,
                        unsigned char* y8_dev, int B, int C, int H, int W, int act_shift, void* stream) {
  return op_groupnorm_fp8(x_dev, gamma_dev, beta_dev, eps, silu, y8_dev, B, C, H, W, act_shift, nullptr, stream);
}
int af_op_groupnorm_fp8_rec(const float* x_dev, const float* gamma_dev, const float* beta_dev, float eps, int silu,
                            unsigned char* y8_dev, int B, int C, int H, int W, int act_shift, void* rec_out_dev, void* stream) {
  if (!rec_out_dev) { af_set_error_msg("af_op_groupnorm_fp8_rec: null record"); return AF_ERR_INVALID; }
  return op_groupnorm_fp8(x_dev, gamma_dev, beta_dev, eps, silu, y8_dev, B, C, H, W, act_shift, reinterpret_cast<unsigned*>(rec_out_dev), stream);
}

// LayerNorm with the e4m3 output the fp8 q / k / v projection reads: y8_dev [rows][C] bytes of result * 2^act_shift
static int op_layernorm_fp8(const float* x_dev, const float* gamma_dev, const float* beta_dev, float eps, unsigned char* y8_dev,
                            int64_t rows, int C, int act_shift, unsigned* rec_out_dev, void* stream) {
  if (!act_shift_ok(act_shift, "af_op_layernorm_fp8")) return AF_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  OP_ALLOC(xn, (size_t)rows * C * 2, false);
  if (rec_out_dev && hipMemsetAsync(rec_out_dev, 0, 2 * sizeof(unsigned), s) != hipSuccess) return AF_ERR_HIP;
  AF_TRY(af_launch_cast_f32<bf16>(x_dev, xn, rows * C, s));
  AF_TRY(af_launch_layernorm<bf16>(xn, C, rows, C, gamma_dev, beta_dev, eps, y8_dev, C, s, ldexpf(1.f, act_shift), rec_out_dev));
  return 0;
}
int af_op_layernorm_fp8(const float* x_dev, const float* gamma_dev, const float* beta_dev, float eps, unsigned char* y8_dev,
                        int64_t rows, int C, int act_shift, void* stream) {
  return op_layernorm_fp8(x_dev, gamma_dev, beta_dev, eps, y8_dev, rows, C, act_shift, nullptr, stream);
}
int af_op_layernorm_fp8_rec(const float* x_dev, const float* gamma_dev, const float* beta_dev, float eps, unsigned char* y8_dev,
                            int64_t rows, int C, int act_shift, void* rec_out_dev, void* stream) {
  if (!rec_out_dev) { af_set_error_msg("af_op_layernorm_fp8_rec: null record"); return AF_ERR_INVALID; }
  return op_layernorm_fp8(x_dev, gamma_dev, beta_dev, eps, y8_dev, rows, C, act_shift, reinterpret_cast<unsigned*>(rec_out_dev), stream);
}

// One FeedForward as the FF scope of the fp8 mode runs it (af_model.hip run_xfmr): e4m3 LayerNorm (or the caller's raw e4m3
// bytes) -> ff_geglu_fp8_kernel -> e4m3 -> the plain fp8 launch with bias / residual / bf16 output.  Weights are repacked to bf16
// and quantised per output row as the model's twins are (af_launch_quant_weight_fp8).
int af_op_ff_fp8(const float* x_dev, const unsigned char* x8_dev, const float* gamma_dev, const float* beta_dev, float eps,
                 const float* w1_dev, const float* b1_dev, const float* w2_dev, const float* b2_dev, const float* residual_dev,
                 int64_t M, int C, int F, int Cout, int shift1, int shift2, void* rec_out_dev, float* y_dev,
                 unsigned char* mid8_dev, int* plan_out, void* stream) {
  if (!act_shift_ok(shift1, "af_op_ff_fp8") || !act_shift_ok(shift2, "af_op_ff_fp8")) return AF_ERR_INVALID;
  if (M <= 0 || M > (1 << 24) || C % 64 != 0 || F % 64 != 0 || Cout % 4 != 0 || !w1_dev || !w2_dev || !y_dev || (!x8_dev && (!x_dev || !gamma_dev || !beta_dev))) {
    af_set_error_msg("af_op_ff_fp8: M=%lld C=%d F=%d Cout=%d (need C%%64==0, F%%64==0, Cout%%4==0, weights, an input)", (long long)M, C, F, Cout);
    return AF_ERR_INVALID;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  const int Mi = (int)M;
  const int rows1 = round_up(2 * F, 128), k1 = round_up(C, 128), rows2 = round_up(Cout, 160), k2 = round_up(F, 128);
  OP_ALLOC(n8, (size_t)M * C, false);
  OP_ALLOC(f8, (size_t)M * F, true);
  OP_ALLOC(w1n, (size_t)rows1 * C * 2, true);
  OP_ALLOC(w18, (size_t)rows1 * k1 + rows1, true);
  OP_ALLOC(w2n, (size_t)rows2 * F * 2, true);
  OP_ALLOC(w28, (size_t)rows2 * k2 + rows2, true);
  OP_ALLOC(yn, (size_t)M * Cout * 2, true);
  OP_ALLOC(b1n, (size_t)rows1 * 4, true);
  OP_ALLOC(b2n, (size_t)rows2 * 4, true);
  unsigned char* sc1 = reinterpret_cast<unsigned char*>(w18) + (size_t)rows1 * k1;
  unsigned char* sc2 = reinterpret_cast<unsigned char*>(w28) + (size_t)rows2 * k2;
  unsigned* rec = reinterpret_cast<unsigned*>(rec_out_dev);
  if (rec && hipMemsetAsync(rec, 0, 2 * sizeof(unsigned), s) != hipSuccess) return AF_ERR_HIP;
  if (x8_dev) {
    if (hipMemcpyAsync(n8, x8_dev, (size_t)M * C, hipMemcpyDeviceToDevice, s) != hipSuccess) return AF_ERR_HIP;
  } else {
    OP_ALLOC(xn, (size_t)M * C * 2, false);
    AF_TRY(af_launch_cast_f32<bf16>(x_dev, xn, M * C, s));
    AF_TRY(af_launch_layernorm<bf16>(xn, C, M, C, gamma_dev, beta_dev, eps, n8, C, s, ldexpf(1.f, shift1), nullptr));
  }
  AF_TRY(af_launch_repack_weight<bf16>(w1_dev, w1n, 2 * F, C, C, 1, C, 0, 1, s));
  AF_TRY(af_launch_quant_weight_fp8(w1n, rows1, C, C, 1, w18, k1, sc1, s));
  AF_TRY(af_launch_repack_weight<bf16>(w2_dev, w2n, Cout, F, F, 1, F, 0, 0, s));
  AF_TRY(af_launch_quant_weight_fp8(w2n, rows2, F, F, 1, w28, k2, sc2, s));
  if (b1_dev) AF_TRY(af_launch_permute_bias(b1_dev, reinterpret_cast<float*>(b1n), 2 * F, 1, s));
  if (b2_dev && hipMemcpyAsync(b2n, b2_dev, (size_t)Cout * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return AF_ERR_HIP;
  void* rn = nullptr;
  if (residual_dev) {
    rn = tmp.get((size_t)M * Cout * 2, false);
    if (!rn) return AF_ERR_HIP;
    AF_TRY(af_launch_cast_f32<bf16>(residual_dev, rn, M * Cout, s));
  }
  ConvGemmParams p;
  memset(&p, 0, sizeof(p));
  p.src = n8; p.src_batch_stride = (long)M * C; p.ldc = C; p.Cin = C;
  p.Hs = 1; p.Ws = Mi; p.Hi = 1; p.Wi = Mi; p.Ho = 1; p.Wo = Mi;
  p.ks = 1; p.stride = 1; p.pad = 0;
  p.W = w18; p.ldw = k1; p.Wrows = rows1;
  p.M = Mi; p.N = 2 * F; p.K = k1; p.k_logical = C;
  p.bias = b1_dev ? reinterpret_cast<float*>(b1n) : nullptr;
  p.out = f8; p.ldo = F; p.alpha = 1.f;
  p.epilogue = AF_EPI_GEGLU;
  p.fp8 = 1; p.w_scale = sc1; p.x_scale_e8 = 127 - shift1;
  if (!af_ff_geglu_fp8_ok(p)) { af_set_error_msg("af_op_ff_fp8: no e4m3 GEGLU launch for M=%d C=%d F=%d", Mi, C, F); return AF_ERR_INVALID; }
  AF_TRY(af_launch_ff_geglu_fp8(p, ldexpf(1.f, shift2), rec, s));
  if (mid8_dev && hipMemcpyAsync(mid8_dev, f8, (size_t)M * F, hipMemcpyDeviceToDevice, s) != hipSuccess) return AF_ERR_HIP;
  ConvGemmParams q;
  memset(&q, 0, sizeof(q));
  q.src = f8; q.src_batch_stride = (long)M * F; q.ldc = F; q.Cin = F;
  q.Hs = 1; q.Ws = Mi; q.Hi = 1; q.Wi = Mi; q.Ho = 1; q.Wo = Mi;
  q.ks = 1; q.stride = 1; q.pad = 0;
  q.W = w28; q.ldw = k2; q.Wrows = rows2;
  q.M = Mi; q.N = Cout; q.K = k2; q.k_logical = F;
  q.bias = b2_dev ? reinterpret_cast<float*>(b2n) : nullptr;
  q.residual = rn; q.ldr = Cout; q.out = yn; q.ldo = Cout; q.alpha = 1.f;
  q.fp8 = 1; q.w_scale = sc2; q.x_scale_e8 = 127 - shift2;
  const AfGemmPlan pl = af_plan_conv_gemm(q, 1, AF_ST_BF16);
  if (pl.kernel != AF_GK_PP_FP8) { af_set_error_msg("af_op_ff_fp8: no fp8 plan for ff.net.2 M=%d N=%d K=%d", q.M, q.N, q.K); return AF_ERR_INVALID; }
  if (plan_out) { plan_out[0] = pl.tile; plan_out[1] = pl.splitk; }
  void* ws = nullptr;
  if (pl.splitk > 1) { ws = tmp.get(pl.ws_bytes, false); if (!ws) return AF_ERR_HIP; }
  AF_TRY(af_launch_conv_gemm<bf16>(q, 1, s, &pl, ws));
  AF_TRY(af_launch_cast_to_f32<bf16>(yn, y_dev, M * Cout, s));
  return 0;
}

// af_op_linear with alpha on the accumulator and row pitches wider than K / N (ld_slack elements, a multiple of 8, added to
// ldc / ldo / ldr; NaN in the slack of the source and the residual, the sentinel in the whole output buffer before the launch).
// ld_slack > 0: y_dev receives the whole rows, float [M][round_up(N, 4) + ld_slack].
int af_op_linear_ex(int dtype, const float* x_dev, const float* w_dev, const float* bias_dev, const float* residual_dev, float alpha,
                    float* y_dev, int64_t M, int K, int N, int geglu, int ld_slack, void* stream) {
  if (ld_slack < 0 || ld_slack % 8 != 0) { af_set_error_msg("af_op_linear_ex: ld_slack must be a non-negative multiple of 8"); return AF_ERR_INVALID; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  const int kp = round_up(K, bk_of(dtype));
  const int rows = geglu ? 2 * N : N;  // weight rows
  const int rows_pad = round_up(rows, 128);
  const int no4 = round_up(N, 4);
  const int ldc = kp + ld_slack, ldo = no4 + ld_slack;
  OP_ALLOC(xn, (size_t)M * ldc * esize(dtype), false);
  OP_ALLOC(wn, (size_t)rows_pad * kp * esize(dtype), true);
  OP_ALLOC(yn, (size_t)M * ldo * esize(dtype), false);
  float* bn = nullptr;
  void* rn = nullptr;
  AF_TRY(fill_cols_dt(dtype, yn, M, ldo, 0, OP_SENTINEL, s));
  // [M,K] rows == NCHW with C=K, HW=1 per "sample": reuse the NCHW converter with B=M, HW=1
  AF_TRY(AF_TYPED(dtype, af_launch_nchw_to_nhwc<Elem>(x_dev, xn, (int)M, K, 1, ldc, 1.f, s)));
  AF_TRY(fill_cols_dt(dtype, xn, M, ldc, kp, OP_NAN, s));
  AF_TRY(AF_TYPED(dtype, af_launch_repack_weight<Elem>(w_dev, wn, rows, K, kp, 1, kp, 0, geglu ? 1 : 0, s)));
  if (bias_dev) {
    bn = reinterpret_cast<float*>(tmp.get((size_t)rows_pad * 4, true));
    if (!bn) return AF_ERR_HIP;
    AF_TRY(af_launch_permute_bias(bias_dev, bn, rows, geglu ? 1 : 0, s));
  }
  if (residual_dev) {
    rn = tmp.get((size_t)M * ldo * esize(dtype), false);
    if (!rn) return AF_ERR_HIP;
    AF_TRY(AF_TYPED(dtype, af_launch_nchw_to_nhwc<Elem>(residual_dev, rn, (int)M, N, 1, ldo, 1.f, s)));
    AF_TRY(fill_cols_dt(dtype, rn, M, ldo, no4, OP_NAN, s));
  }
  ConvGemmParams p;
  memset(&p, 0, sizeof(p));
  p.src = xn; p.src_batch_stride = (long)M * ldc; p.ldc = ldc; p.Cin = kp;
  p.Hs = 1; p.Ws = (int)M; p.Hi = 1; p.Wi = (int)M; p.Ho = 1; p.Wo = (int)M;
  p.ks = 1; p.stride = 1; p.pad = 0;
  p.W = wn; p.ldw = kp; p.Wrows = rows_pad;
  p.M = (int)M; p.N = geglu ? 2 * N : no4; p.K = kp;
  p.bias = bn; p.residual = rn; p.ldr = ldo; p.out = yn; p.ldo = ldo;
  p.epilogue = geglu ? AF_EPI_GEGLU : AF_EPI_NONE;
  p.alpha = alpha;
  p.k_logical = K;
  const AfGemmPlan pl = af_plan_conv_gemm(p, 1, storage_of(dtype));
  void* ws = nullptr;
  if (pl.splitk > 1) { ws = tmp.get(pl.ws_bytes, false); if (!ws) return AF_ERR_HIP; }
  AF_TRY(AF_TYPED(dtype, af_launch_conv_gemm<Elem>(p, 1, s, &pl, ws)));
  if (ld_slack > 0) {
    AF_TRY(AF_TYPED(dtype, af_launch_cast_to_f32<Elem>(yn, y_dev, M * ldo, s)));
    return 0;
  }
  AF_TRY(AF_TYPED(dtype, af_launch_nhwc_to_nchw<Elem>(yn, y_dev, (int)M, N, 1, no4, s)));
  return 0;
}
int af_op_linear(int dtype, const float* x_dev, const float* w_dev, const float* bias_dev, const float* residual_dev,
                 float* y_dev, int64_t M, int K, int N, int geglu, void* stream) {
  return af_op_linear_ex(dtype, x_dev, w_dev, bias_dev, residual_dev, 1.f, y_dev, M, K, N, geglu, 0, stream);
}

// GroupNorm (no SiLU) followed by a 1x1 convolution -- SpatialTransformer.norm + proj_in (attention.py:325-326) -- both ways
// on the same bf16 operands: y_plain = the apply pass + the GEMM, y_fused = the row-panel GEMM normalising its rows in its
// prologue (ConvGemmParams::gn_ab).  Outputs [B, N, H, W] fp32.  Fails when the shape has no row-panel launch.
int af_op_gn_conv1x1(const float* x_dev, const float* gamma_dev, const float* beta_dev, float eps, const float* w_dev,
                     const float* bias_dev, float* y_plain_dev, float* y_fused_dev, int B, int C, int H, int W, int N,
                     void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  const int HW = H * W, rows_pad = round_up(N, 128);
  if (C % 64 || N % 4) { af_set_error_msg("af_op_gn_conv1x1: C %% 64 and N %% 4"); return AF_ERR_INVALID; }
  OP_ALLOC(xn, (size_t)B * HW * C * 2, false);
  OP_ALLOC(gn, (size_t)B * HW * C * 2, false);
  OP_ALLOC(wn, (size_t)rows_pad * C * 2, true);
  OP_ALLOC(y0, (size_t)B * HW * N * 2, true);
  OP_ALLOC(y1, (size_t)B * HW * N * 2, true);
  OP_ALLOC(ws, af_gn_workspace_bytes(B, HW), false);
  OP_ALLOC(ab, (size_t)B * 2 * C * sizeof(float), false);
  float* bn = nullptr;
  if (bias_dev) {
    bn = reinterpret_cast<float*>(tmp.get((size_t)rows_pad * 4, true));
    if (!bn) return AF_ERR_HIP;
    if (hipMemcpyAsync(bn, bias_dev, (size_t)N * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return AF_ERR_HIP;
  }
  AF_TRY(af_launch_nchw_to_nhwc<bf16>(x_dev, xn, B, C, HW, C, 1.f, s));
  AF_TRY(af_launch_repack_weight<bf16>(w_dev, wn, N, C, C, 1, C, 0, 0, s));
  ConvGemmParams p;
  memset(&p, 0, sizeof(p));
  p.src_batch_stride = (long)HW * C; p.ldc = C; p.Cin = C;
  p.Hs = H; p.Ws = W; p.Hi = H; p.Wi = W; p.Ho = H; p.Wo = W;
  p.ks = 1; p.stride = 1; p.pad = 0;
  p.W = wn; p.ldw = C; p.Wrows = rows_pad;
  p.M = B * HW; p.N = N; p.K = C; p.k_logical = C;
  p.bias = bn; p.ldo = N; p.alpha = 1.f;
  // plain: GroupNorm apply pass, then the GEMM as the planner places it
  AF_TRY(af_launch_groupnorm<bf16>(xn, (long)HW * C, C, B, HW, C, gamma_dev, beta_dev, eps, 0, gn, (long)HW * C, C, ws, s));
  {
    ConvGemmParams q = p;
    q.src = gn; q.out = y0;
    const AfGemmPlan pl = af_plan_conv_gemm(q, 1, AF_ST_BF16);
    void* wsk = nullptr;
    if (pl.splitk > 1) { wsk = tmp.get(pl.ws_bytes, false); if (!wsk) return AF_ERR_HIP; }
    AF_TRY(af_launch_conv_gemm<bf16>(q, 1, s, &pl, wsk));
  }
  // fused: statistics + fold, the GEMM reads the un-normalised rows
  AF_TRY(af_launch_groupnorm_fold<bf16>(xn, (long)HW * C, C, B, HW, C, gamma_dev, beta_dev, eps, ws, s, nullptr, 0, (float*)ab));
  {
    ConvGemmParams q = p;
    q.src = xn; q.out = y1;
    q.gn_ab = (const float*)ab; q.gn_hw = HW;
    const AfGemmPlan pl = af_plan_conv_gemm(q, 1, AF_ST_BF16);
    if (pl.kernel != AF_GK_ROWPANEL) { af_set_error_msg("af_op_gn_conv1x1: M=%d K=%d N=%d has no row-panel launch", q.M, q.K, q.N); return AF_ERR_INVALID; }
    AF_TRY(af_launch_conv_gemm<bf16>(q, 1, s, &pl, nullptr));
  }
  AF_TRY(af_launch_nhwc_to_nchw<bf16>(y0, y_plain_dev, B, N, HW, N, s));
  AF_TRY(af_launch_nhwc_to_nchw<bf16>(y1, y_fused_dev, B, N, HW, N, s));
  return 0;
}

// One producer GEMM -> LayerNorm -> consumer GEMM pair of a transformer block with the LayerNorm folded into the two GEMMs, on
// the launches run_xfmr (af_model.hip) makes, every intermediate returned: t = a Wp^T + bp + res with ln_stats_out, the folded
// consumer weight (af_launch_ln_fold), the consumer on the partial sums or on finalised statistics as af_ln_consumer_stats
// (af_host.h, Runner::conv's own decision) says, and the unfolded route (af_launch_layernorm on t, then the plain GEMM) beside
// it.  Both launches are planned on aligned dummies first, so a shape that cannot fold is refused before the device is touched.
// Test hooks: the sentinel in the whole t and y buffers (guard_rows rows behind the M valid ones included) and NaN in all
// parts_cap slabs before the launches.
int af_op_ln_chain(int dtype, const float* a_dev, const float* wp_dev, const float* bp_dev, const float* res_dev,
                   const float* gamma_dev, const float* beta_dev, float eps, const float* wc_dev, const float* bc_dev, int64_t M,
                   int Kp, int C, int N, int geglu, int parts_n, int parts_cap, int guard_rows, float* wf_dev, float* colsum_dev,
                   float* biasf_dev, float* t_dev, float* parts_dev, float* stats_dev, float* y_folded_dev, float* y_plain_dev,
                   int* plans10, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype != AF_DTYPE_BF16) {
    af_set_error_msg("af_op_ln_chain: LayerNorm-fused launches exist for bf16 storage only (dtype %d)", dtype);
    return AF_ERR_INVALID;
  }
  const int rows = geglu ? 2 * N : N;   // consumer weight rows
  if (M <= 0 || M + guard_rows > 0x7fffffff || guard_rows < 0 || Kp <= 0 || Kp % 64 != 0 || C <= 0 || C % 64 != 0 || N <= 0 ||
      N % 4 != 0 || (geglu && rows % 64 != 0) || parts_cap <= 0) {
    af_set_error_msg("af_op_ln_chain: M=%lld Kp=%d C=%d N=%d geglu=%d (Kp, C: multiples of 64; N: of 4, GEGLU: of 32)", (long long)M,
                     Kp, C, N, geglu);
    return AF_ERR_INVALID;
  }
  const int rows_pad_p = round_up(C, 128), rows_pad_c = round_up(rows, 128);
  const long Mg = (long)M + guard_rows;
  alignas(16) static char dummy[16];
  ConvGemmParams pp, pc;
  memset(&pp, 0, sizeof(pp));
  pp.src = dummy; pp.src_batch_stride = (long)M * Kp; pp.ldc = Kp; pp.Cin = Kp;
  pp.Hs = 1; pp.Ws = (int)M; pp.Hi = 1; pp.Wi = (int)M; pp.Ho = 1; pp.Wo = (int)M;
  pp.ks = 1; pp.stride = 1; pp.pad = 0;
  pp.W = dummy; pp.ldw = Kp; pp.Wrows = rows_pad_p;
  pp.M = (int)M; pp.N = C; pp.K = Kp; pp.k_logical = Kp;
  pp.bias = bp_dev ? reinterpret_cast<const float*>(dummy) : nullptr;
  pp.residual = res_dev ? dummy : nullptr; pp.ldr = C;
  pp.out = dummy; pp.ldo = C; pp.alpha = 1.f;
  pp.ln_stats_out = reinterpret_cast<float*>(dummy);
  pc = pp;
  pc.src_batch_stride = (long)M * C; pc.ldc = C; pc.Cin = C;
  pc.ldw = C; pc.Wrows = rows_pad_c;
  pc.N = rows; pc.K = C; pc.k_logical = C;
  pc.bias = reinterpret_cast<const float*>(dummy);
  pc.residual = nullptr; pc.ldr = 0;
  pc.ldo = N;
  pc.epilogue = geglu ? AF_EPI_GEGLU : AF_EPI_NONE;
  pc.ln_stats_out = nullptr;
  pc.ln_stats = reinterpret_cast<const float*>(dummy); pc.ln_colsum = reinterpret_cast<const float*>(dummy);
  ConvGemmParams pu = pc;   // the unfolded consumer
  pu.ln_stats = nullptr; pu.ln_colsum = nullptr;
  pu.bias = bc_dev ? reinterpret_cast<const float*>(dummy) : nullptr;
  // the model's refusals (xfmr_ln_parts): both launches must plan a LayerNorm epilogue -- asked as Runner::ln_capable asks, of the
  // launch without its LayerNorm arguments and residual -- and the consumer is handed the producer's slab count
  int slabs = 0;
  {
    ConvGemmParams qa = pp, qb = pc;
    qa.ln_stats_out = nullptr; qa.residual = nullptr; qa.ldr = 0;
    qb.ln_stats = nullptr; qb.ln_colsum = nullptr;
    const AfGemmPlan a = af_plan_conv_gemm(qa, 1, AF_ST_BF16), b = af_plan_conv_gemm(qb, 1, AF_ST_BF16);
    slabs = a.ln_slabs;
    if (a.ln_slabs <= 0 || b.ln_slabs <= 0) {
      af_set_error_msg("af_op_ln_chain: the %s [%lld, %d] -> %d plans no LayerNorm epilogue (kernel %d, %d K slices)",
                       a.ln_slabs <= 0 ? "producer" : "consumer", (long long)M, a.ln_slabs <= 0 ? Kp : C, a.ln_slabs <= 0 ? C : rows,
                       a.ln_slabs <= 0 ? a.kernel : b.kernel, a.ln_slabs <= 0 ? a.splitk : b.splitk);
      return AF_ERR_INVALID;
    }
    if (af_plan_conv_gemm(pp, 1, AF_ST_BF16).ln_slabs != slabs || af_plan_conv_gemm(pc, 1, AF_ST_BF16).ln_slabs <= 0) {
      af_set_error_msg("af_op_ln_chain: the launches with their LayerNorm arguments plan other statistics slabs than the bare ones (%d)", slabs);
      return AF_ERR_INVALID;
    }
    if ((parts_n > 0 ? parts_n : a.ln_slabs) != a.ln_slabs) {
      af_set_error_msg("af_op_ln_chain: the producer writes %d statistics slabs, the consumer is handed %d", a.ln_slabs, parts_n);
      return AF_ERR_INVALID;
    }
    if (a.ln_slabs > parts_cap) {
      af_set_error_msg("af_op_ln_chain: %d statistics slabs, room for %d", a.ln_slabs, parts_cap);
      return AF_ERR_INVALID;
    }
  }
  Tmp tmp;
  OP_ALLOC(an, (size_t)M * Kp * 2, false);
  OP_ALLOC(wpn, (size_t)rows_pad_p * Kp * 2, true);
  OP_ALLOC(wcn, (size_t)rows_pad_c * C * 2, true);
  OP_ALLOC(wcf, (size_t)rows_pad_c * C * 2, true);
  OP_ALLOC(cs, (size_t)rows_pad_c * 4, true);
  OP_ALLOC(bf, (size_t)rows_pad_c * 4, true);
  OP_ALLOC(tn, (size_t)Mg * C * 2, false);
  OP_ALLOC(tl, (size_t)M * C * 2, false);
  OP_ALLOC(y0, (size_t)Mg * N * 2, false);
  OP_ALLOC(y1, (size_t)Mg * N * 2, false);
  OP_ALLOC(parts, (size_t)parts_cap * M * 2 * sizeof(float), false);
  OP_ALLOC(st_own, (size_t)M * 2 * sizeof(float), true);
  OP_ALLOC(st_tap, (size_t)M * 2 * sizeof(float), true);
  float *bpn = nullptr, *bcn = nullptr;
  void* rn = nullptr;
  AF_TRY(fill_cols_dt(dtype, tn, Mg, C, 0, OP_SENTINEL, s));
  AF_TRY(fill_cols_dt(dtype, y0, Mg, N, 0, OP_SENTINEL, s));
  AF_TRY(fill_cols_dt(dtype, y1, Mg, N, 0, OP_SENTINEL, s));
  AF_TRY(fill_cols_dt(AF_DTYPE_F32, parts, (long)parts_cap * M, 2, 0, OP_NAN, s));
  AF_TRY(af_launch_cast_f32<bf16>(a_dev, an, (long)M * Kp, s));
  AF_TRY(af_launch_repack_weight<bf16>(wp_dev, wpn, C, Kp, Kp, 1, Kp, 0, 0, s));
  AF_TRY(af_launch_repack_weight<bf16>(wc_dev, wcn, rows, C, C, 1, C, 0, geglu ? 1 : 0, s));
  if (bp_dev) {
    bpn = reinterpret_cast<float*>(tmp.get((size_t)rows_pad_p * 4, true));
    if (!bpn) return AF_ERR_HIP;
    AF_TRY(af_launch_permute_bias(bp_dev, bpn, C, 0, s));
  }
  if (bc_dev) {
    bcn = reinterpret_cast<float*>(tmp.get((size_t)rows_pad_c * 4, true));
    if (!bcn) return AF_ERR_HIP;
    AF_TRY(af_launch_permute_bias(bc_dev, bcn, rows, geglu ? 1 : 0, s));
  }
  if (res_dev) {
    rn = tmp.get((size_t)M * C * 2, false);
    if (!rn) return AF_ERR_HIP;
    AF_TRY(af_launch_cast_f32<bf16>(res_dev, rn, (long)M * C, s));
  }
  AF_TRY(af_launch_ln_fold<bf16>(wcn, wcf, gamma_dev, beta_dev, bcn, (float*)cs, (float*)bf, rows_pad_c, C, C, s));
  // producer
  pp.src = an; pp.W = wpn; pp.bias = bpn; pp.residual = rn; pp.out = tn;
  pp.ln_stats_out = (float*)parts;
  const AfGemmPlan plp = af_plan_conv_gemm(pp, 1, AF_ST_BF16);
  // folded consumer: planned with the finalised statistics' buffer, which af_ln_consumer_stats fills or replaces
  pc.src = tn; pc.W = wcf; pc.bias = (const float*)bf; pc.out = y1;
  pc.ln_colsum = (const float*)cs; pc.ln_stats = (const float*)st_own;
  const AfGemmPlan plc = af_plan_conv_gemm(pc, 1, AF_ST_BF16);
  if (plp.ln_slabs != slabs || plc.ln_slabs <= 0) {
    af_set_error_msg("af_op_ln_chain: the launches as stated plan %d / %d statistics slabs, the bare ones %d", plp.ln_slabs,
                     plc.ln_slabs, slabs);
    return AF_ERR_INVALID;
  }
  AF_TRY(af_launch_conv_gemm<bf16>(pp, 1, s, &plp, nullptr));
  AF_TRY(af_launch_ln_finalize((const float*)parts, slabs, (int)M, C, eps, (float*)st_tap, s));
  AF_TRY(af_ln_consumer_stats(pc, plc, (const float*)parts, slabs, C, eps, (float*)st_own, false, s));
  AF_TRY(af_launch_conv_gemm<bf16>(pc, 1, s, &plc, nullptr));
  // the unfolded route on the same t
  AF_TRY(af_launch_layernorm<bf16>(tn, C, (long)M, C, gamma_dev, beta_dev, eps, tl, C, s));
  pu.src = tl; pu.W = wcn; pu.bias = bcn; pu.out = y0;
  {
    const AfGemmPlan pl = af_plan_conv_gemm(pu, 1, AF_ST_BF16);
    void* wsk = nullptr;
    if (pl.splitk > 1) { wsk = tmp.get(pl.ws_bytes, false); if (!wsk) return AF_ERR_HIP; }
    AF_TRY(af_launch_conv_gemm<bf16>(pu, 1, s, &pl, wsk));
  }
  if (plans10) {
    const int o[10] = {plp.kernel, plp.rowpanel, plp.tile, plp.splitk, plp.ln_slabs, plc.kernel, plc.rowpanel, plc.tile, plc.splitk, plc.ln_slabs};
    memcpy(plans10, o, sizeof(o));
  }
  if (wf_dev) AF_TRY(af_launch_cast_to_f32<bf16>(wcf, wf_dev, (long)rows * C, s));
  if (colsum_dev) HIP_CHECK_RET(hipMemcpyAsync(colsum_dev, cs, (size_t)rows * 4, hipMemcpyDeviceToDevice, s));
  if (biasf_dev) HIP_CHECK_RET(hipMemcpyAsync(biasf_dev, bf, (size_t)rows * 4, hipMemcpyDeviceToDevice, s));
  if (t_dev) AF_TRY(af_launch_cast_to_f32<bf16>(tn, t_dev, Mg * C, s));
  if (parts_dev) HIP_CHECK_RET(hipMemcpyAsync(parts_dev, parts, (size_t)parts_cap * M * 2 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (stats_dev) HIP_CHECK_RET(hipMemcpyAsync(stats_dev, st_tap, (size_t)M * 2 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (y_folded_dev) AF_TRY(af_launch_cast_to_f32<bf16>(y1, y_folded_dev, Mg * N, s));
  if (y_plain_dev) AF_TRY(af_launch_cast_to_f32<bf16>(y0, y_plain_dev, Mg * N, s));
  return 0;
}

int af_op_groupnorm(int dtype, const float* x_dev, const float* gamma_dev, const float* beta_dev, float eps, int silu,
                    float* y_dev, int B, int C, int H, int W, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  const int HW = H * W;
  // (a shape the launcher would refuse is refused here, before the layout conversion: nothing is allocated or launched)
  if (af_plan_groupnorm(storage_of(dtype), B, HW, C, 0).kernel == AF_GNK_REFUSED) {
    af_set_error_msg("af_op_groupnorm: unsupported B=%d C=%d %dx%d", B, C, H, W);
    return AF_ERR_INVALID;
  }
  OP_ALLOC(xn, (size_t)B * HW * C * esize(dtype), false);
  OP_ALLOC(yn, (size_t)B * HW * C * esize(dtype), false);
  OP_ALLOC(ws, af_gn_workspace_bytes(B, HW), false);
  AF_TRY(AF_TYPED(dtype, af_launch_nchw_to_nhwc<Elem>(x_dev, xn, B, C, HW, C, 1.f, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_groupnorm<Elem>(xn, (long)HW * C, C, B, HW, C, gamma_dev, beta_dev, eps, silu, yn,
                                                   (long)HW * C, C, ws, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_nhwc_to_nchw<Elem>(yn, y_dev, B, C, HW, C, s)));
  return 0;
}

// 3x3 / stride-1 convolution (bf16) followed by GroupNorm(32) (+SiLU) as a ResBlock runs the pair: the convolution also
// writes the GroupNorm partial sums of its output (ConvGemmParams::gn_stats_out) and the GroupNorm makes no statistics pass.
// h_dev: the convolution's output, y_dev: the GroupNorm's; AF_ERR_INVALID when the shape has no producer plan.
int af_op_conv_gn(const float* x_dev, const float* w_dev, const float* bias_dev, const float* residual_dev,
                  const float* gamma_dev, const float* beta_dev, float eps, int silu, float* h_dev, float* y_dev, int B,
                  int Cin, int H, int W, int Cout, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  if (Cin % 64 != 0 || Cout % 32 != 0) { af_set_error_msg("af_op_conv_gn: Cin%%64==0 and Cout%%32==0"); return AF_ERR_INVALID; }
  const int HW = H * W, rows_pad = round_up(Cout, 128), ldw = 9 * Cin;
  OP_ALLOC(xn, (size_t)B * HW * Cin * 2, false);
  OP_ALLOC(wn, (size_t)rows_pad * ldw * 2, true);
  OP_ALLOC(hn, (size_t)B * HW * Cout * 2, true);
  OP_ALLOC(yn, (size_t)B * HW * Cout * 2, false);
  OP_ALLOC(ws, af_gn_workspace_bytes(B, HW), false);
  OP_ALLOC(st, (size_t)B * (HW / 64 + 1) * 32 * 2 * sizeof(float), true);
  void* rn = nullptr;
  float* bn = nullptr;
  AF_TRY(af_launch_nchw_to_nhwc<bf16>(x_dev, xn, B, Cin, HW, Cin, 1.f, s));
  AF_TRY(af_launch_repack_weight<bf16>(w_dev, wn, Cout, Cin, Cin, 3, ldw, 0, 0, s));
  if (bias_dev) {
    bn = reinterpret_cast<float*>(tmp.get((size_t)rows_pad * 4, true));
    if (!bn) return AF_ERR_HIP;
    if (hipMemcpyAsync(bn, bias_dev, (size_t)Cout * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return AF_ERR_HIP;
  }
  if (residual_dev) {
    rn = tmp.get((size_t)B * HW * Cout * 2, false);
    if (!rn) return AF_ERR_HIP;
    AF_TRY(af_launch_nchw_to_nhwc<bf16>(residual_dev, rn, B, Cout, HW, Cout, 1.f, s));
  }
  ConvGemmParams p;
  memset(&p, 0, sizeof(p));
  p.src = xn; p.src_batch_stride = (long)HW * Cin; p.ldc = Cin; p.Cin = Cin;
  p.Hs = H; p.Ws = W; p.Hi = H; p.Wi = W; p.Ho = H; p.Wo = W;
  p.ks = 3; p.stride = 1; p.pad = 1;
  p.W = wn; p.ldw = ldw; p.Wrows = rows_pad;
  p.M = B * HW; p.N = Cout; p.K = ldw;
  p.bias = bn; p.residual = rn; p.ldr = Cout; p.out = hn; p.ldo = Cout; p.alpha = 1.f;
  p.k_logical = 9 * Cin;
  const AfGemmPlan pl = af_plan_conv_gemm(p, 1, AF_ST_BF16);
  if (!af_conv_gn_stats_ok(p, pl, Cout / 32)) {
    af_set_error_msg("af_op_conv_gn: no GroupNorm-statistics producer plan for M=%d N=%d K=%d", p.M, p.N, p.K);
    return AF_ERR_INVALID;
  }
  p.gn_stats_out = reinterpret_cast<float*>(st);
  p.gn_cpg = Cout / 32;
  AF_TRY(af_launch_conv_gemm<bf16>(p, 1, s, &pl, nullptr));
  AF_TRY(af_launch_groupnorm<bf16>(hn, (long)HW * Cout, Cout, B, HW, Cout, gamma_dev, beta_dev, eps, silu, yn, (long)HW * Cout,
                                   Cout, ws, s, 0.f, reinterpret_cast<const float*>(st), HW / 64));
  AF_TRY(af_launch_nhwc_to_nchw<bf16>(hn, h_dev, B, Cout, HW, Cout, s));
  AF_TRY(af_launch_nhwc_to_nchw<bf16>(yn, y_dev, B, Cout, HW, Cout, s));
  return 0;
}

int af_op_layernorm(int dtype, const float* x_dev, const float* gamma_dev, const float* beta_dev, float eps,
                    float* y_dev, int64_t rows, int C, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  if (af_plan_layernorm(storage_of(dtype), rows, C).kernel == AF_LNK_REFUSED) {   // (before the cast: nothing is launched)
    af_set_error_msg("af_op_layernorm: unsupported C=%d", C);
    return AF_ERR_INVALID;
  }
  OP_ALLOC(xn, (size_t)rows * C * esize(dtype), false);
  OP_ALLOC(yn, (size_t)rows * C * esize(dtype), false);
  AF_TRY(AF_TYPED(dtype, af_launch_cast_f32<Elem>(x_dev, xn, rows * C, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_layernorm<Elem>(xn, C, rows, C, gamma_dev, beta_dev, eps, yn, C, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_cast_to_f32<Elem>(yn, y_dev, rows * C, s)));
  return 0;
}

// af_op_attention in the forms of AttnParams only the model states (Runner::attn_params, af_model.hip): q | k | v as columns of
// one [B][N][3C] buffer (layout AF_ATTN_QKV), k | v as columns of the cached context [B][Nk][2C] with the V^T pack made from it
// (AF_ATTN_CTX), row pitches wider than the channel count (ld_slack), a log-sum-exp output, a window [b0, b0 + nb) of the batch
// and a key list cut short (drop_keys).  Test hooks, always on: every input buffer holds 0xFF bytes (NaN) wherever no operand
// is -- slack columns, 128 tail rows -- and the output buffer and lse_dev hold them before the launch; o_dev receives the whole
// pitched output, float [B][Nq][C + ld_slack].
int af_op_attention_ex(int dtype, const float* q_dev, const float* k_dev, const float* v_dev, float* o_dev, float* lse_dev, int B,
                       int Nq, int Nk, int heads, int dh, float scale, int flags, int layout, int ld_slack, int b0, int nb,
                       int drop_keys, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  if (nb < 0) nb = B - b0;
  if ((dtype != AF_DTYPE_BF16 && dtype != AF_DTYPE_F32 && dtype != AF_DTYPE_F16) || !q_dev || !k_dev || !v_dev || !o_dev || B <= 0 ||
      Nq <= 0 || Nk <= 0 || heads <= 0 || dh <= 0 || dh % 8 || layout < AF_ATTN_DENSE || layout > AF_ATTN_CTX || ld_slack < 0 ||
      ld_slack % 8 || b0 < 0 || nb < 0 || b0 + nb > B || drop_keys < 0 || drop_keys >= Nk || (layout == AF_ATTN_QKV && Nq != Nk)) {
    af_set_error_msg("af_op_attention_ex: dtype=%d B=%d Nq=%d Nk=%d heads=%d dh=%d layout=%d ld_slack=%d window (%d, %d) drop_keys=%d "
                     "(dh and ld_slack multiples of 8; the qkv layout needs Nq == Nk)", dtype, B, Nq, Nk, heads, dh, layout, ld_slack,
                     b0, nb, drop_keys);
    return AF_ERR_INVALID;
  }
  const bool causal = (flags & 1) != 0;
  const size_t es = esize(dtype);
  const int C = heads * dh, nkeys = Nk - drop_keys;
  const int ldo = C + ld_slack;
  const int ldq = (layout == AF_ATTN_QKV ? 3 * C : C) + ld_slack;
  const int ldk = (layout == AF_ATTN_QKV ? 3 * C : layout == AF_ATTN_CTX ? 2 * C : C) + ld_slack;
  const long rq = (long)B * Nq, rk = (long)B * Nk, tail_rows = 128;
  // a [rows + 128 tail rows][ld] buffer of NaN bytes
  auto nan_buf = [&](long rows, int ld) -> void* {
    const size_t bytes = (size_t)(rows + tail_rows) * ld * es;
    void* b = tmp.get(bytes, false);
    if (b && hipMemsetAsync(b, 0xFF, bytes, s) != hipSuccess) return nullptr;   // 0xFFFF / 0xFFFFFFFF: NaN
    return b;
  };
  // fp32 [rows][C] -> columns [off, off + C) of a [rows][ld] buffer of the storage type
  auto put = [&](const float* src, long rows, void* dst, int ld, int off) -> int {
    void* dense = tmp.get((size_t)rows * C * es, false);
    if (!dense) { af_set_error_msg("hipMalloc failed in op"); return AF_ERR_HIP; }
    AF_TRY(AF_TYPED(dtype, af_launch_cast_f32<Elem>(src, dense, rows * C, s)));
    AF_TRY(AF_TYPED(dtype, af_launch_copy_channels<Elem>(dense, C, dst, ld, off, C, rows, s)));
    return 0;
  };
  void *qn = nullptr, *kn = nullptr, *vn = nullptr;
  if (layout == AF_ATTN_QKV) {
    qn = nan_buf(rq, ldq);
    if (!qn) { af_set_error_msg("hipMalloc failed in op"); return AF_ERR_HIP; }
    kn = (char*)qn + (size_t)C * es;
    vn = (char*)qn + (size_t)2 * C * es;
  } else {
    qn = nan_buf(rq, ldq);
    kn = nan_buf(rk, ldk);
    vn = layout == AF_ATTN_CTX ? (kn ? (void*)((char*)kn + (size_t)C * es) : nullptr) : nan_buf(rk, ldk);
    if (!qn || !kn || !vn) { af_set_error_msg("hipMalloc failed in op"); return AF_ERR_HIP; }
  }
  AF_TRY(put(q_dev, rq, qn, ldq, 0));
  AF_TRY(put(k_dev, rk, layout == AF_ATTN_QKV ? qn : kn, ldk, layout == AF_ATTN_QKV ? C : 0));
  AF_TRY(put(v_dev, rk, layout == AF_ATTN_DENSE ? vn : layout == AF_ATTN_QKV ? qn : kn, ldk, layout == AF_ATTN_DENSE ? 0 : layout == AF_ATTN_QKV ? 2 * C : C));
  const size_t o_bytes = (size_t)rq * ldo * es;
  OP_ALLOC(on, o_bytes, false);
  if (hipMemsetAsync(on, 0xFF, o_bytes, s) != hipSuccess) return AF_ERR_HIP;
  if (lse_dev && hipMemsetAsync(lse_dev, 0xFF, (size_t)B * heads * Nq * sizeof(float), s) != hipSuccess) return AF_ERR_HIP;
  // the window: as Runner::attn_params moves the pointers
  AttnParams p;
  p.ldq = ldq; p.ldk = p.ldv = ldk; p.ldo = ldo;
  p.bsq = (long)Nq * ldq; p.bso = (long)Nq * ldo; p.bsk = p.bsv = (long)Nk * ldk;
  p.q = (char*)qn + (size_t)b0 * p.bsq * es; p.k = (char*)kn + (size_t)b0 * p.bsk * es;
  p.v = (char*)vn + (size_t)b0 * p.bsv * es; p.o = (char*)on + (size_t)b0 * p.bso * es;
  p.lse = lse_dev ? lse_dev + (size_t)b0 * heads * Nq : nullptr;
  p.causal = causal ? 1 : 0;
  p.Nq = Nq; p.Nk = nkeys; p.H = heads; p.scale = scale;
  p.vt_pack = nullptr;
  if (dtype == AF_DTYPE_BF16 && !causal && !lse_dev && layout != AF_ATTN_QKV) {   // as af_set_context does for the cached cross-attention K / V
    const long pe = af_attn_short_pack_elems<bf16>(B, heads, dh, nkeys);
    if (pe > 0) {
      OP_ALLOC(vt, (size_t)pe * 2, false);
      AF_TRY(af_launch_attn_short_pack<bf16>(vn, ldk, p.bsv, nkeys, heads, dh, B, vt, s));
      p.vt_pack = (char*)vt + (size_t)b0 * (size_t)(pe / B) * 2;
    }
  }
  AF_TRY(AF_TYPED(dtype, af_launch_attention<Elem>(p, nb, dh, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_cast_to_f32<Elem>(on, o_dev, rq * ldo, s)));
  return 0;
}
int af_op_attention(int dtype, const float* q_dev, const float* k_dev, const float* v_dev, float* o_dev, int B, int Nq,
                    int Nk, int heads, int dh, float scale, int causal, void* stream) {   // causal = flags: bit 0 causal, bit 1 NaN guard rows
  return af_op_attention_ex(dtype, q_dev, k_dev, v_dev, o_dev, nullptr, B, Nq, Nk, heads, dh, scale, causal, AF_ATTN_DENSE, 0, 0, -1, 0,
                            stream);
}

// ---- regional prompts (af_region_attn.hip) ----
int af_region_plan_query(int dtype, int dh, int T, int R, int64_t* out) {
  if (!out || (dtype != AF_DTYPE_BF16 && dtype != AF_DTYPE_F32 && dtype != AF_DTYPE_F16)) {
    af_set_error_msg("af_region_plan_query: bad argument");
    return AF_ERR_INVALID;
  }
  *out = af_plan_region_attention(storage_of(dtype), dh, T, R);
  return AF_OK;
}
int64_t af_region_attn_launches(void) { return g_af_region_attn_launches; }

int af_op_region_weights(const float* m_dev, int Bf, int R, int H, int W, float* out_pyramid_dev, uint32_t* out_bits_dev,
                         void* stream) {
  if (!m_dev || !out_pyramid_dev || !out_bits_dev) { af_set_error_msg("af_op_region_weights: null argument"); return AF_ERR_INVALID; }
  return af_launch_region_weights(m_dev, Bf, R, H, W, out_pyramid_dev, out_bits_dev, reinterpret_cast<hipStream_t>(stream))
             ? AF_ERR_INVALID : AF_OK;
}

// The regional attention on either path, staged as the model holds its operands: K | V as columns of one [B][R T][2C + slack]
// buffer, q and o with the same slack, NaN bytes wherever no operand is (as af_op_attention_ex).
int af_op_region_attention(int dtype, const float* q_dev, const float* k_dev, const float* v_dev, const float* w_dev, float* o_dev,
                           int B, int Nq, int R, int T, int heads, int dh, float scale, int path, int ld_slack, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  if ((dtype != AF_DTYPE_BF16 && dtype != AF_DTYPE_F32 && dtype != AF_DTYPE_F16) || !q_dev || !k_dev || !v_dev || !w_dev || !o_dev ||
      B <= 0 || Nq <= 0 || T <= 0 || heads <= 0 || dh <= 0 || dh % 8 || ld_slack < 0 || ld_slack % 8 || path < 0 || path > 2) {
    af_set_error_msg("af_op_region_attention: dtype=%d B=%d Nq=%d R=%d T=%d heads=%d dh=%d path=%d ld_slack=%d (dh and ld_slack "
                     "multiples of 8; path 0 planner, 1 composition, 2 fused)", dtype, B, Nq, R, T, heads, dh, path, ld_slack);
    return AF_ERR_INVALID;
  }
  int plan = af_plan_region_attention(storage_of(dtype), dh, T, R);
  if (plan == AF_RGK_REFUSED) {
    af_set_error_msg("af_op_region_attention: refused (1 .. %d regions, head dim 8, 16, 32, 40, 64, 80, 128 or 160), got R=%d dh=%d",
                     AF_REGION_MAX, R, dh);
    return AF_ERR_INVALID;
  }
  if (path == 1) plan = AF_RGK_COMPOSE;
  if (path == 2) {
    if (AF_TYPED(dtype, af_region_pack_elems<Elem>(B, R, heads, dh, T)) <= 0) {
      af_set_error_msg("af_op_region_attention: no fused kernel for dtype %d, head dim %d, %d keys per segment", dtype, dh, T);
      return AF_ERR_INVALID;
    }
    plan = AF_RGK_FUSED;
  }
  const size_t es = esize(dtype);
  const int C = heads * dh, S = R * T;
  const int ldq = C + ld_slack, ldo = C + ld_slack, ldk = 2 * C + ld_slack;
  const long rq = (long)B * Nq, rk = (long)B * S, tail_rows = 128;
  auto nan_buf = [&](long rows, int ld) -> void* {
    const size_t bytes = (size_t)(rows + tail_rows) * ld * es;
    void* b = tmp.get(bytes, false);
    if (b && hipMemsetAsync(b, 0xFF, bytes, s) != hipSuccess) return nullptr;
    return b;
  };
  auto put = [&](const float* src, long rows, void* dst, int ld, int off) -> int {
    void* dense = tmp.get((size_t)rows * C * es, false);
    if (!dense) { af_set_error_msg("hipMalloc failed in op"); return AF_ERR_HIP; }
    AF_TRY(AF_TYPED(dtype, af_launch_cast_f32<Elem>(src, dense, rows * C, s)));
    AF_TRY(AF_TYPED(dtype, af_launch_copy_channels<Elem>(dense, C, dst, ld, off, C, rows, s)));
    return 0;
  };
  void* qn = nan_buf(rq, ldq);
  void* kn = nan_buf(rk, ldk);
  if (!qn || !kn) { af_set_error_msg("hipMalloc failed in op"); return AF_ERR_HIP; }
  void* vn = (char*)kn + (size_t)C * es;
  AF_TRY(put(q_dev, rq, qn, ldq, 0));
  AF_TRY(put(k_dev, rk, kn, ldk, 0));
  AF_TRY(put(v_dev, rk, kn, ldk, C));
  const size_t o_bytes = (size_t)rq * ldo * es;
  OP_ALLOC(on, o_bytes, false);
  if (hipMemsetAsync(on, 0xFF, o_bytes, s) != hipSuccess) return AF_ERR_HIP;
  if (plan == AF_RGK_FUSED) {
    // the active bits of every 32-query block, from w (host: an operator for tests)
    const int nblk = (Nq + 31) / 32;
    std::vector<float> wh((size_t)B * R * Nq);
    HIP_CHECK_RET(hipMemcpyAsync(wh.data(), w_dev, wh.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    std::vector<unsigned> bh((size_t)B * nblk, 0u);
    for (int b = 0; b < B; ++b)
      for (int r = 0; r < R; ++r)
        for (int q = 0; q < Nq; ++q)
          if (wh[((size_t)b * R + r) * Nq + q] > 0.f) bh[(size_t)b * nblk + q / 32] |= 1u << r;
    OP_ALLOC(bits, bh.size() * sizeof(unsigned), false);
    HIP_CHECK_RET(hipMemcpyAsync(bits, bh.data(), bh.size() * sizeof(unsigned), hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));   // (`bh` is a pageable host temporary)
    const long pe = AF_TYPED(dtype, af_region_pack_elems<Elem>(B, R, heads, dh, T));
    OP_ALLOC(vt, (size_t)pe * es, false);
    AF_TRY(AF_TYPED(dtype, af_launch_region_pack<Elem>(vn, ldk, (long)S * ldk, T, R, heads, dh, B, vt, s)));
    AfRegionAttnArgs a;
    a.q = qn; a.k = kn; a.o = on; a.vt = vt; a.w = w_dev; a.bits = reinterpret_cast<const unsigned*>(bits);
    a.ldq = ldq; a.ldk = ldk; a.ldo = ldo; a.bsq = (long)Nq * ldq; a.bsk = (long)S * ldk; a.bso = (long)Nq * ldo;
    a.B = B; a.Nq = Nq; a.R = R; a.T = T; a.heads = heads; a.dh = dh; a.scale = scale; a.level = 0;
    AF_TRY(AF_TYPED(dtype, af_launch_region_attention<Elem>(a, s)));
  } else {
    // R launches of the attention kernels on the key segments (a pointer offset of r T rows, the batch stride of the whole
    // list) into R dense outputs, then the combine
    OP_ALLOC(parts, (size_t)R * rq * C * es + 4096, false);
    for (int r = 0; r < R; ++r) {
      AttnParams p;
      p.ldq = ldq; p.ldk = p.ldv = ldk; p.ldo = C;
      p.bsq = (long)Nq * ldq; p.bso = (long)Nq * C; p.bsk = p.bsv = (long)S * ldk;
      p.q = qn; p.k = (char*)kn + (size_t)r * T * ldk * es; p.v = (char*)vn + (size_t)r * T * ldk * es;
      p.o = (char*)parts + (size_t)r * rq * C * es;
      p.lse = nullptr; p.causal = 0; p.Nq = Nq; p.Nk = T; p.H = heads; p.scale = scale; p.vt_pack = nullptr;
      AF_TRY(AF_TYPED(dtype, af_launch_attention<Elem>(p, B, dh, s)));
    }
    AF_TRY(AF_TYPED(dtype, af_launch_region_combine<Elem>(parts, rq * C, w_dev, on, ldo, B, Nq, C, R, s)));
  }
  AF_TRY(AF_TYPED(dtype, af_launch_cast_to_f32<Elem>(on, o_dev, rq * ldo, s)));
  return 0;
}

// Host-only diagnostic: the kernel af_launch_attention would run (AfAttnKernel); no device is touched
int af_attn_plan_query(int dtype, int dh, int Nk, int ldq, int ldk, int ldv, int ldo, int flags, int64_t* out) {
  if (!out || (dtype != AF_DTYPE_BF16 && dtype != AF_DTYPE_F32 && dtype != AF_DTYPE_F16)) {
    af_set_error_msg("af_attn_plan_query: bad argument");
    return AF_ERR_INVALID;
  }
  *out = af_plan_attention(storage_of(dtype), dh, Nk, ldq, ldk, ldv, ldo, (flags & AF_AQ_CAUSAL) != 0, (flags & AF_AQ_LSE) != 0,
                           (flags & AF_AQ_VT_PACK) != 0);
  return AF_OK;
}

// Cross-attention with subject-token conv attention, on the launches xfmr_cross_attention_conv (af_model.hip) makes for a run of
// samples that all carry n_groups subject strings at the end of their key list.
int af_op_conv_attention(int dtype, const float* q_dev, const float* k_dev, const float* v_dev, float* o_dev, int B, int Hh,
                         int Ww, int Nk, int heads, int dh, float scale, int ks, int n_groups, int path, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  if (!q_dev || !k_dev || !v_dev || !o_dev || B <= 0 || Hh <= 0 || Ww <= 0 || heads <= 0 || dh <= 0 || dh > 160 || dh % 8 ||
      ks < 2 || ks > 4 || n_groups <= 0 || n_groups * ks * ks >= Nk || path < 0 || path > 2) {
    af_set_error_msg("af_op_conv_attention: B=%d map %dx%d Nk=%d heads=%d dh=%d ks=%d groups=%d path=%d", B, Hh, Ww, Nk, heads,
                     dh, ks, n_groups, path);
    return AF_ERR_INVALID;
  }
  const int C = heads * dh, N = Hh * Ww, nt = ks * ks;
  const long nq = (long)B * N * C, nk = (long)B * Nk * C;
  const bool bf = dtype == AF_DTYPE_BF16;
  const long pe = bf ? af_attn_short_pack_elems<bf16>(B, heads, dh, Nk) : 0;
  const bool can = af_conv_attn_short_ok(bf, dh, Nk, pe > 0, ks, n_groups);
  if (path == 2 && !can) {
    af_set_error_msg("af_op_conv_attention: no one-pass kernel for dtype %d, dh %d, %d keys, ks %d, %d subject strings (bf16, dh 40 / 80, "
                     "<= 96 keys)", dtype, dh, Nk, ks, n_groups);
    return AF_ERR_INVALID;
  }
  const bool one_pass = path == 2 || (path == 0 && can && g_af_knobs.conv_attn_short && g_af_knobs.attn_short);
  OP_ALLOC(qn, (size_t)nq * esize(dtype), false);
  OP_ALLOC(kn, (size_t)nk * esize(dtype), false);
  OP_ALLOC(vn, (size_t)nk * esize(dtype), false);
  OP_ALLOC(kvn, (size_t)2 * nk * esize(dtype), false);   // K | V rows, as the cached context
  OP_ALLOC(on, (size_t)nq * esize(dtype), true);
  AF_TRY(AF_TYPED(dtype, af_launch_cast_f32<Elem>(q_dev, qn, nq, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_cast_f32<Elem>(k_dev, kn, nk, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_cast_f32<Elem>(v_dev, vn, nk, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_copy_channels<Elem>(kn, C, kvn, 2 * C, 0, C, (long)B * Nk, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_copy_channels<Elem>(vn, C, kvn, 2 * C, C, C, (long)B * Nk, s)));
  AttnParams p;
  p.q = qn; p.k = kvn; p.v = (char*)kvn + (size_t)C * esize(dtype); p.o = on; p.lse = nullptr; p.causal = 0;
  p.ldq = C; p.ldo = C; p.ldk = p.ldv = 2 * C;
  p.bsq = p.bso = (long)N * C; p.bsk = p.bsv = (long)Nk * 2 * C;
  p.Nq = N; p.Nk = Nk; p.H = heads; p.scale = scale;
  p.vt_pack = nullptr;
  if (one_pass) {
    OP_ALLOC(vt, (size_t)pe * 2, false);
    OP_ALLOC(amap, af_conv_attn_map_floats(n_groups, B, heads, N) * sizeof(float), false);
    AF_TRY(af_launch_attn_short_pack<bf16>(p.v, 2 * C, (long)Nk * 2 * C, Nk, heads, dh, B, vt, s));
    p.vt_pack = vt;
    AF_TRY(af_launch_conv_attn_map<bf16>(qn, C, (long)N * C, kvn, 2 * C, (long)Nk * 2 * C, Nk - n_groups * nt, n_groups,
                                         (float*)amap, B, heads, dh, Hh, Ww, ks, s));
    AF_TRY(af_launch_conv_attn_short(p, B, dh, ks, n_groups, Hh, Ww, (const float*)amap, s));
  } else {
    OP_ALLOC(lse, (size_t)B * heads * N * sizeof(float), false);
    OP_ALLOC(s9, (size_t)B * heads * N * nt * sizeof(float), false);
    p.lse = (float*)lse;
    p.Nk = Nk - n_groups * nt;
    AF_TRY(AF_TYPED(dtype, af_launch_attention<Elem>(p, B, dh, s)));
    for (int g = 0; g < n_groups; ++g) {
      const int tok0 = Nk - (n_groups - g) * nt;
      AF_TRY(AF_TYPED(dtype, af_launch_conv_attn<Elem>(qn, C, (long)N * C, kvn, 2 * C, (long)Nk * 2 * C, tok0, (float*)s9,
                                                       (float*)lse, on, C, (long)N * C, B, N, heads, dh, Hh, Ww, scale, ks, s)));
    }
  }
  AF_TRY(AF_TYPED(dtype, af_launch_cast_to_f32<Elem>(on, o_dev, nq, s)));
  return 0;
}

// The VAE AttnBlock between its qkv convolution and proj_out, on the launches run_vae_attn (af_model.hip) makes: q | k | v
// interleaved into one [B][N][3C] buffer, then af_vae_attn_core.  Test hooks around the core: 128 rows of NaN behind the qkv
// buffer (a ragged tile of the last sample's K rows must be zero-filled, not read), the sentinel in the whole scores, V^T and
// output buffers before the run and in 4 KiB behind each of them, which must still hold it afterwards.
int af_op_vae_attention(int dtype, const float* q_dev, const float* k_dev, const float* v_dev, float* o_dev, int B, int N, int C,
                        float* scores_dev, float* probs_dev, int* plans6, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  if ((dtype != AF_DTYPE_BF16 && dtype != AF_DTYPE_F32 && dtype != AF_DTYPE_F16) || !q_dev || !k_dev || !v_dev || !o_dev ||
      B <= 0 || N <= 0 || C <= 0 || C % bk_of(dtype) != 0 || (double)B * N * std::max(N, C) >= 1073741824.0) {
    af_set_error_msg("af_op_vae_attention: dtype=%d B=%d N=%d C=%d (C: a multiple of the K tile; B * N * max(N, C) below 2^30)", dtype, B,
                     N, C);
    return AF_ERR_INVALID;
  }
  if (!af_vae_attn_shape_ok(dtype, N)) return AF_ERR_INVALID;   // (before anything is allocated or launched)
  const size_t es = esize(dtype), guard = 4096;
  const long nx = (long)B * N * C, nn = (long)B * N * N, ng = (long)(guard / es);
  const size_t tail = (size_t)128 * 3 * C * es;
  OP_ALLOC(qn, (size_t)nx * es, false);
  OP_ALLOC(kn, (size_t)nx * es, false);
  OP_ALLOC(vn, (size_t)nx * es, false);
  OP_ALLOC(qkv, (size_t)3 * nx * es + tail, false);
  OP_ALLOC(sc, (size_t)nn * es + guard, false);
  OP_ALLOC(vt, (size_t)nx * es + guard, false);
  OP_ALLOC(on, (size_t)nx * es + guard, false);
  HIP_CHECK_RET(hipMemsetAsync((char*)qkv + (size_t)3 * nx * es, 0xFF, tail, s));   // 0xFFFF / 0xFFFFFFFF: NaN
  AF_TRY(fill_cols_dt(dtype, sc, 1, (int)(nn + ng), 0, OP_SENTINEL, s));
  AF_TRY(fill_cols_dt(dtype, vt, 1, (int)(nx + ng), 0, OP_SENTINEL, s));
  AF_TRY(fill_cols_dt(dtype, on, 1, (int)(nx + ng), 0, OP_SENTINEL, s));
  AF_TRY(AF_TYPED(dtype, af_launch_cast_f32<Elem>(q_dev, qn, nx, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_cast_f32<Elem>(k_dev, kn, nx, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_cast_f32<Elem>(v_dev, vn, nx, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_copy_channels<Elem>(qn, C, qkv, 3 * C, 0, C, (long)B * N, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_copy_channels<Elem>(kn, C, qkv, 3 * C, C, C, (long)B * N, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_copy_channels<Elem>(vn, C, qkv, 3 * C, 2 * C, C, (long)B * N, s)));
  AfVaeAttnTaps taps;
  memset(&taps, 0, sizeof(taps));
  if (scores_dev) { taps.scores = tmp.get((size_t)nn * es); if (!taps.scores) return AF_ERR_HIP; }
  if (probs_dev) { taps.probs = tmp.get((size_t)nn * es); if (!taps.probs) return AF_ERR_HIP; }
  void* const guards[3] = {(char*)sc + (size_t)nn * es, (char*)vt + (size_t)nx * es, (char*)on + (size_t)nx * es};
  static const char* const guard_names[3] = {"scores", "V^T", "output"};
  std::vector<unsigned char> before(3 * guard), after(3 * guard);
  for (int i = 0; i < 3; ++i) HIP_CHECK_RET(hipMemcpyAsync(before.data() + i * guard, guards[i], guard, hipMemcpyDeviceToHost, s));
  AF_TRY(af_vae_attn_core(dtype, qkv, sc, vt, on, B, N, C, s, &taps));
  for (int i = 0; i < 3; ++i) HIP_CHECK_RET(hipMemcpyAsync(after.data() + i * guard, guards[i], guard, hipMemcpyDeviceToHost, s));
  HIP_CHECK_RET(hipStreamSynchronize(s));
  for (int i = 0; i < 3; ++i)
    for (size_t j = 0; j < guard; ++j)
      if (before[i * guard + j] != after[i * guard + j]) {
        af_set_error_msg("af_op_vae_attention: byte %zu behind the %s buffer was written (B=%d N=%d C=%d dtype=%d)", j, guard_names[i],
                         B, N, C, dtype);
        return AF_ERR_STATE;
      }
  if (plans6) memcpy(plans6, taps.plans, sizeof(taps.plans));
  if (scores_dev) AF_TRY(AF_TYPED(dtype, af_launch_cast_to_f32<Elem>(taps.scores, scores_dev, nn, s)));
  if (probs_dev) AF_TRY(AF_TYPED(dtype, af_launch_cast_to_f32<Elem>(taps.probs, probs_dev, nn, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_cast_to_f32<Elem>(on, o_dev, nx, s)));
  return 0;
}

// One cross-attention layer through xattn_fused_kernel (bf16), prepared as the model prepares it: LayerNorm folded into to_q
// (af_launch_ln_fold), K / V packed per head pair, to_out's K dimension permuted.  ln_parts_out_dev (optional): [4][B * N][2]
// partial sums of the stored rows, as the next LayerNorm's consumer reads them.
int af_op_xattn_fused(const float* x_dev, const float* ln_stats_dev, const float* gamma_dev, const float* beta_dev,
                      const float* wq_dev, const float* kv_dev, const float* wo_dev, const float* bo_dev, float* y_dev,
                      float* ln_parts_out_dev, int B, int N, int S, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  constexpr int C = 320, Hh = 8, dh = 40;
  const int M = B * N, rows_pad = round_up(C, 128);
  if (!af_xattn_fused_ok(M, N, C, Hh, dh, S)) { af_set_error_msg("af_op_xattn_fused: B=%d N=%d S=%d has no fused kernel", B, N, S); return AF_ERR_INVALID; }
  OP_ALLOC(xn, (size_t)M * C * 2, false);
  OP_ALLOC(yn, (size_t)M * C * 2, true);
  OP_ALLOC(wq, (size_t)rows_pad * C * 2, true);
  OP_ALLOC(wqf, (size_t)rows_pad * C * 2, true);
  OP_ALLOC(wo, (size_t)rows_pad * C * 2, true);
  OP_ALLOC(wop, (size_t)rows_pad * C * 2, true);
  OP_ALLOC(cs, (size_t)rows_pad * 4, true);
  OP_ALLOC(bf, (size_t)rows_pad * 4, true);
  OP_ALLOC(kvn, (size_t)B * S * 2 * C * 2, false);
  const long pe = af_xattn_fused_pack_elems(B, Hh, dh, S);
  OP_ALLOC(pack, (size_t)pe * 2, false);
  OP_ALLOC(parts, (size_t)4 * M * 2 * sizeof(float), true);
  AF_TRY(af_launch_cast_f32<bf16>(x_dev, xn, (long)M * C, s));
  AF_TRY(af_launch_cast_f32<bf16>(kv_dev, kvn, (long)B * S * 2 * C, s));
  AF_TRY(af_launch_repack_weight<bf16>(wq_dev, wq, C, C, C, 1, C, 0, 0, s));
  AF_TRY(af_launch_repack_weight<bf16>(wo_dev, wo, C, C, C, 1, C, 0, 0, s));
  AF_TRY(af_launch_ln_fold<bf16>(wq, wqf, gamma_dev, beta_dev, nullptr, (float*)cs, (float*)bf, rows_pad, C, C, s));
  AF_TRY(af_launch_xattn_fused_permute_wo(wo, C, C, wop, C, s));
  AF_TRY(af_launch_xattn_fused_pack(kvn, 2 * C, (long)S * 2 * C, S, B, pack, s));
  AfXattnFusedParams a;
  memset(&a, 0, sizeof(a));
  a.x = xn; a.ldx = C; a.M = M; a.rows_per_sample = N;
  a.ln_stats = ln_stats_dev; a.ln_parts_n = 0;
  a.wq = wqf; a.ldwq = C; a.q_colsum = (const float*)cs; a.q_bias = (const float*)bf;
  a.kvpack = pack;
  a.wo = wop; a.ldwo = C; a.o_bias = bo_dev;
  a.out = yn; a.ldo = C;
  a.ln_stats_out = (float*)parts;
  a.Nk = S;
  AF_TRY(af_launch_xattn_fused(a, s));
  AF_TRY(af_launch_cast_to_f32<bf16>(yn, y_dev, (long)M * C, s));
  if (ln_parts_out_dev && hipMemcpyAsync(ln_parts_out_dev, parts, (size_t)4 * M * 2 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
    return AF_ERR_HIP;
  return 0;
}

// Token merging (af_tome.hip), the launches xfmr_self_attention_tome makes
static bool tome_dtype_ok(int dtype, const char* who) {
  if (dtype == AF_DTYPE_BF16 || dtype == AF_DTYPE_F32) return true;
  af_set_error_msg("%s: storage type %d (token merging takes bf16 and f32)", who, dtype);
  return false;
}
int af_op_tome_match(int dtype, const float* x_dev, int B, int H, int W, int C, double ratio, int normalize, int32_t* node_idx_dev,
                     float* node_max_dev, int32_t* map_dev, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  AfTomePlan pl;
  if (!tome_dtype_ok(dtype, "af_op_tome_match") || af_tome_plan(H, W, ratio, &pl)) return AF_ERR_INVALID;
  if (B <= 0 || C <= 0 || !x_dev || !node_idx_dev || !node_max_dev || !map_dev) { af_set_error_msg("af_op_tome_match: bad argument"); return AF_ERR_INVALID; }
  const long n = (long)B * H * W * C;
  OP_ALLOC(xn, (size_t)n * esize(dtype), false);
  OP_ALLOC(ws, af_tome_match_ws_bytes(B, H, W), false);
  AF_TRY(AF_TYPED(dtype, af_launch_cast_f32<Elem>(x_dev, xn, n, s)));
  const int rc = dtype == AF_DTYPE_BF16
                     ? af_launch_tome_match<bf16>(xn, C, B, H, W, C, ratio, normalize, node_idx_dev, node_max_dev, map_dev, ws, s)
                     : af_launch_tome_match<float>(xn, C, B, H, W, C, ratio, normalize, node_idx_dev, node_max_dev, map_dev, ws, s);
  return rc ? AF_ERR_INVALID : AF_OK;
}
int af_op_tome_merge(int dtype, const float* x_dev, const float* gamma_dev, const float* beta_dev, float eps,
                     const int32_t* map_dev, int B, int N, int Nprime, int C, float* y_dev, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  if (!tome_dtype_ok(dtype, "af_op_tome_merge")) return AF_ERR_INVALID;
  if (B <= 0 || N <= 0 || Nprime <= 0 || Nprime > N || C <= 0 || !x_dev || !map_dev || !y_dev) { af_set_error_msg("af_op_tome_merge: bad argument"); return AF_ERR_INVALID; }
  const long nx = (long)B * N * C, ny = (long)B * Nprime * C;
  OP_ALLOC(xn, (size_t)nx * esize(dtype), false);
  OP_ALLOC(yn, (size_t)ny * esize(dtype), true);
  AF_TRY(AF_TYPED(dtype, af_launch_cast_f32<Elem>(x_dev, xn, nx, s)));
  const int rc = dtype == AF_DTYPE_BF16
                     ? af_launch_tome_merge<bf16>(xn, C, gamma_dev, beta_dev, eps, map_dev, B, N, Nprime, C, yn, C, s)
                     : af_launch_tome_merge<float>(xn, C, gamma_dev, beta_dev, eps, map_dev, B, N, Nprime, C, yn, C, s);
  if (rc) return AF_ERR_INVALID;
  AF_TRY(AF_TYPED(dtype, af_launch_cast_to_f32<Elem>(yn, y_dev, ny, s)));
  return AF_OK;
}
int af_op_tome_unmerge_add(int dtype, const float* o_dev, const float* res_dev, const int32_t* map_dev, int B, int N, int Nprime,
                           int C, float* y_dev, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  if (!tome_dtype_ok(dtype, "af_op_tome_unmerge_add")) return AF_ERR_INVALID;
  if (B <= 0 || N <= 0 || Nprime <= 0 || Nprime > N || C <= 0 || !o_dev || !res_dev || !map_dev || !y_dev) { af_set_error_msg("af_op_tome_unmerge_add: bad argument"); return AF_ERR_INVALID; }
  const long no = (long)B * Nprime * C, ny = (long)B * N * C;
  OP_ALLOC(on, (size_t)no * esize(dtype), false);
  OP_ALLOC(rn, (size_t)ny * esize(dtype), false);
  OP_ALLOC(yn, (size_t)ny * esize(dtype), true);
  AF_TRY(AF_TYPED(dtype, af_launch_cast_f32<Elem>(o_dev, on, no, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_cast_f32<Elem>(res_dev, rn, ny, s)));
  const int rc = dtype == AF_DTYPE_BF16
                     ? af_launch_tome_unmerge_add<bf16>(on, C, rn, C, map_dev, B, N, Nprime, C, yn, C, nullptr, 0, s)
                     : af_launch_tome_unmerge_add<float>(on, C, rn, C, map_dev, B, N, Nprime, C, yn, C, nullptr, 0, s);
  if (rc) return AF_ERR_INVALID;
  AF_TRY(AF_TYPED(dtype, af_launch_cast_to_f32<Elem>(yn, y_dev, ny, s)));
  return AF_OK;
}

// FreeU on one concatenation (af_freeu.hip): the buffer [B][H W][Ch + Cs] as the model holds it, the model's launcher, and back
int af_op_freeu(int dtype, const float* h_dev, const float* skip_dev, int B, int Ch, int Cs, int H, int W, int version, double b,
                double s, float* h_out_dev, float* skip_out_dev, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  if (dtype != AF_DTYPE_BF16 && dtype != AF_DTYPE_F32 && dtype != AF_DTYPE_F16) { af_set_error_msg("af_op_freeu: storage type %d", dtype); return AF_ERR_INVALID; }
  if (B <= 0 || !h_dev || !skip_dev || !h_out_dev || !skip_out_dev) { af_set_error_msg("af_op_freeu: bad argument"); return AF_ERR_INVALID; }
  if (!(b >= 1.0 && b <= 2.0) || !(s >= 0.0 && s <= 1.0)) { af_set_error_msg("af_op_freeu: b %g outside [1, 2] or s %g outside [0, 1]", b, s); return AF_ERR_INVALID; }
  AfFreeuPlan pl;
  if (af_plan_freeu(H, W, Ch, Cs, version, &pl)) return AF_ERR_INVALID;
  const int HW = H * W, ld = Ch + Cs;
  const long npix = (long)B * HW;
  OP_ALLOC(hn, (size_t)npix * Ch * esize(dtype), false);
  OP_ALLOC(sn, (size_t)npix * Cs * esize(dtype), false);
  OP_ALLOC(cat, (size_t)npix * ld * esize(dtype) + 4096, false);
  OP_ALLOC(ws, af_freeu_ws_bytes(B, H, W, Ch, Cs, version), false);
  AF_TRY(AF_TYPED(dtype, af_launch_nchw_to_nhwc<Elem>(h_dev, hn, B, Ch, HW, Ch, 1.0f, st)));
  AF_TRY(AF_TYPED(dtype, af_launch_nchw_to_nhwc<Elem>(skip_dev, sn, B, Cs, HW, Cs, 1.0f, st)));
  AF_TRY(AF_TYPED(dtype, af_launch_copy_channels<Elem>(hn, Ch, cat, ld, 0, Ch, npix, st)));
  AF_TRY(AF_TYPED(dtype, af_launch_copy_channels<Elem>(sn, Cs, cat, ld, Ch, Cs, npix, st)));
  if (AF_TYPED(dtype, af_launch_freeu<Elem>(cat, ld, B, H, W, Ch, Cs, version, (float)b, (float)s, true, true, ws, st))) return AF_ERR_INVALID;
  AF_TRY(AF_TYPED(dtype, af_launch_nhwc_to_nchw<Elem>(cat, h_out_dev, B, Ch, HW, ld, st)));
  AF_TRY(AF_TYPED(dtype, af_launch_nhwc_to_nchw<Elem>(reinterpret_cast<char*>(cat) + (size_t)Ch * esize(dtype), skip_out_dev, B, Cs, HW, ld, st)));
  return AF_OK;
}

// The LoRA-merging weight repack (af_lora.hip) on caller-owned buffers: dst_dev holds elements of `dtype` and is written in place
int af_op_lora_repack(int dtype, const float* base_dev, int rows, int cin, int cin_pad, int ks, int ldw, int row_off, int perm,
                      int n_adapters, const float* const* up_dev, const float* const* down_dev, const int* ranks,
                      const float* scales, void* dst_dev, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype != AF_DTYPE_BF16 && dtype != AF_DTYPE_F32 && dtype != AF_DTYPE_F16) { af_set_error_msg("af_op_lora_repack: storage type %d", dtype); return AF_ERR_INVALID; }
  AF_TRY(AF_TYPED(dtype, af_launch_lora_repack<Elem>(base_dev, dst_dev, rows, cin, cin_pad, ks, ldw, row_off, perm != 0, n_adapters,
                                                     up_dev, down_dev, ranks, scales, s)));
  return AF_OK;
}

// The T-GATE add (af_tgate.hip) on caller-owned buffers of `dtype` elements, rows and strides as given
int af_op_tgate_add(int dtype, const void* t1_dev, const void* src_dev, void* t2_dev, void* cache_dev, float* stats_dev, int parts,
                    int L, int B, int N, int C, int ld_t1, int ld_src, int ld_t2, int ld_cache, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype != AF_DTYPE_BF16 && dtype != AF_DTYPE_F32 && dtype != AF_DTYPE_F16) { af_set_error_msg("af_op_tgate_add: storage type %d", dtype); return AF_ERR_INVALID; }
  if (B <= 0) { af_set_error_msg("af_op_tgate_add: bad argument"); return AF_ERR_INVALID; }
  if (AF_TYPED(dtype, af_launch_tgate_add<Elem>(t1_dev, ld_t1, src_dev, ld_src, t2_dev, ld_t2, cache_dev, ld_cache, L, B, N, C,
                                                stats_dev, parts, s)))
    return AF_ERR_INVALID;
  return AF_OK;
}

// The attention-mass kernel of self-attention guidance (af_sag.hip) on caller-owned q / k of `dtype` elements: [B][N][ld], the
// first heads * dh columns of a row are the operand (column views of a wider buffer pass their first element and its row stride);
// part_dev: fp32 scratch of B * heads * N values (the per-head column sums)
int af_op_sag_mass(int dtype, const void* q_dev, const void* k_dev, float* mass_dev, float* part_dev, int B, int N, int heads, int dh,
                   int ld_q, int ld_k, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype != AF_DTYPE_BF16 && dtype != AF_DTYPE_F32 && dtype != AF_DTYPE_F16) { af_set_error_msg("af_op_sag_mass: storage type %d", dtype); return AF_ERR_INVALID; }
  if (B <= 0) { af_set_error_msg("af_op_sag_mass: bad argument"); return AF_ERR_INVALID; }
  const int rc = AF_TYPED(dtype, af_launch_sag_mass<Elem>(q_dev, ld_q, (long)N * ld_q, k_dev, ld_k, (long)N * ld_k, mass_dev, part_dev, B, N, heads,
                                                          dh, s));
  return rc == 0 ? AF_OK : rc == -2 ? AF_ERR_HIP : AF_ERR_INVALID;
}

// The ControlNet residual add (af_controlnet.hip) on caller-owned buffers of `dtype` elements: one launch for all n segments
int af_op_control_add(int dtype, int n, void* const* dst_dev, const void* const* src_dev, const int* C, const int* ld,
                      const int64_t* rows_per_sample, const float* scales, int Bs, int Bd, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype != AF_DTYPE_BF16 && dtype != AF_DTYPE_F32 && dtype != AF_DTYPE_F16) { af_set_error_msg("af_op_control_add: storage type %d", dtype); return AF_ERR_INVALID; }
  if (n < 1 || n > AF_CONTROL_MAX_SEGMENTS) { af_set_error_msg("af_op_control_add: %d segments (1 .. %d)", n, (int)AF_CONTROL_MAX_SEGMENTS); return AF_ERR_INVALID; }
  if (!dst_dev || !src_dev || !C || !ld || !rows_per_sample || !scales) { af_set_error_msg("af_op_control_add: null argument"); return AF_ERR_INVALID; }
  if (Bs <= 0 || (Bd != Bs && Bd != 2 * Bs)) { af_set_error_msg("af_op_control_add: dst batch %d for a src batch of %d (equal, or twice it)", Bd, Bs); return AF_ERR_INVALID; }
  AfControlSeg segs[AF_CONTROL_MAX_SEGMENTS];
  for (int k = 0; k < n; ++k) {
    if (rows_per_sample[k] <= 0) { af_set_error_msg("af_op_control_add: segment %d has %lld rows per sample", k, (long long)rows_per_sample[k]); return AF_ERR_INVALID; }
    segs[k] = AfControlSeg{dst_dev[k], src_dev[k], (long)Bs * rows_per_sample[k], C[k], ld[k], scales[k]};
  }
  if (AF_TYPED(dtype, af_launch_control_add<Elem>(segs, n, s))) return AF_ERR_INVALID;
  return AF_OK;
}

int af_op_timestep_embedding(int dtype, const int64_t* t_dev, float* y_dev, int B, int dim, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Tmp tmp;
  OP_ALLOC(yn, (size_t)B * dim * esize(dtype), false);
  AF_TRY(AF_TYPED(dtype, af_launch_timestep_embedding<Elem>((const long long*)t_dev, yn, B, dim, s)));
  AF_TRY(AF_TYPED(dtype, af_launch_cast_to_f32<Elem>(yn, y_dev, (long)B * dim, s)));
  return 0;
}

}  // extern "C"
