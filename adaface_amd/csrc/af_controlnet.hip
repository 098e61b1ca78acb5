// adaface_amd — ControlNet: Zhang, Rao, Agrawala, "Adding Conditional Control to Text-to-Image Diffusion Models"
// (ICCV 2023).  The control branch itself is the U-Net encoder's own kernels under a second set of weights (af_model.hip); the one
// thing it adds to the hot path is the injection of its residuals into the main U-Net's skip connections, here:
//   dst_k[r][0 .. C_k) = round(dst_k[r][c] + round32(s_k * src_k[r][c]))       for every row r < rows_k of up to 16 segments
// in ONE launch.  dst_k is a channel range of a concatenation buffer (row stride ld_k >= C_k elements), src_k is dense.  The
// product and the sum are two fp32 operations, each rounded (never contracted into an fma), then the storage type's one rounding
// to nearest even: the result is the same bits on every path.  Nothing outside [0, C_k) of a row is read or written.
// The segment table travels by value in the kernel arguments; a block finds its segment in the prefix table of block counts and
// walks that segment's 16-byte vectors (or elements, where a pointer or a row stride does not allow vectors) with a grid stride
// of the segment's own blocks.
#include "af_kernels.h"

#include <algorithm>
#include <cstring>

// No contraction in this file: hipcc contracts a * b + c into an fma by default (and its __fmul_rn / __fadd_rn are inline
// functions compiled under that default, so they contract as well).  The product below must be rounded before the sum: the
// arithmetic is written with plain operators under this pragma.
#pragma clang fp contract(off)

std::atomic<long> g_af_control_add_launches{0};

namespace controlnet {

struct Seg {
  void* dst;
  const void* src;
  long rows;
  int C, ld;
  float scale;
  int vec;   // 1: 16-byte accesses
};
struct Table {
  Seg seg[AF_CONTROL_MAX_SEGMENTS];
  unsigned blk_end[AF_CONTROL_MAX_SEGMENTS];   // blocks of segments 0 .. k
  int n;
};

constexpr int kThreads = 256;
constexpr int kItemsPerThread = 4;     // vectors a thread aims to handle: 16 KiB of each operand per block
constexpr unsigned kMaxBlocksPerSeg = 1024;

// fl(d + fl(s * r)): the product is rounded to fp32 before the sum (see the pragma above)
__device__ __forceinline__ float add_scaled(float d, float s, float r) {
  const float p = s * r;
  return d + p;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void control_add_kernel(const Table tb) {
  constexpr int EPC = 16 / (int)sizeof(T);
  int k = 0;
  while (k + 1 < tb.n && blockIdx.x >= tb.blk_end[k]) ++k;
  const Seg sg = tb.seg[k];
  const unsigned first = k ? tb.blk_end[k - 1] : 0u;
  const long nblk = (long)(tb.blk_end[k] - first);
  const long stride = nblk * kThreads;
  const float s = sg.scale;
  T* __restrict__ dst = reinterpret_cast<T*>(sg.dst);
  const T* __restrict__ src = reinterpret_cast<const T*>(sg.src);
  if (sg.vec) {
    const int NV = sg.C / EPC;
    const long total = sg.rows * NV;
    for (long v = (long)(blockIdx.x - first) * kThreads + threadIdx.x; v < total; v += stride) {
      const long row = v / NV;
      const int col = (int)(v - row * NV) * EPC;
      Vec16<T> d, r;
      r.u = *reinterpret_cast<const uint4*>(src + row * sg.C + col);
      d.u = *reinterpret_cast<const uint4*>(dst + row * sg.ld + col);
#pragma unroll
      for (int e = 0; e < EPC; ++e) d.e[e] = from_f32<T>(add_scaled(to_f32<T>(d.e[e]), s, to_f32<T>(r.e[e])));
      *reinterpret_cast<uint4*>(dst + row * sg.ld + col) = d.u;
    }
  } else {
    const long total = sg.rows * sg.C;
    for (long v = (long)(blockIdx.x - first) * kThreads + threadIdx.x; v < total; v += stride) {
      const long row = v / sg.C;
      const int col = (int)(v - row * sg.C);
      T* d = dst + row * sg.ld + col;
      *d = from_f32<T>(add_scaled(to_f32<T>(*d), s, to_f32<T>(src[row * sg.C + col])));
    }
  }
}

}  // namespace controlnet

template <typename T>
int af_launch_control_add(const AfControlSeg* segs, int n, hipStream_t s) {
  using namespace controlnet;
  constexpr int EPC = 16 / (int)sizeof(T);
  if (n < 0 || n > AF_CONTROL_MAX_SEGMENTS || (n && !segs)) { af_set_error_msg("control add: %d segments (at most %d)", n, AF_CONTROL_MAX_SEGMENTS); return -1; }
  Table tb;
  memset(&tb, 0, sizeof(tb));
  unsigned blocks = 0;
  double bytes = 0.0;
  auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  for (int k = 0; k < n; ++k) {
    const AfControlSeg& a = segs[k];
    if (!a.dst || !a.src) { af_set_error_msg("control add: segment %d has a null operand", k); return -1; }
    if (a.rows < 0 || a.C <= 0 || a.ld < a.C) { af_set_error_msg("control add: segment %d: rows %ld, C %d, row stride %d", k, a.rows, a.C, a.ld); return -1; }
    if (!(a.scale == a.scale) || a.scale - a.scale != 0.f) { af_set_error_msg("control add: segment %d: scale is not finite", k); return -1; }
    if (a.rows == 0) continue;
    Seg& g = tb.seg[tb.n];
    g.dst = a.dst; g.src = a.src; g.rows = a.rows; g.C = a.C; g.ld = a.ld; g.scale = a.scale;
    g.vec = (a.C % EPC == 0 && a.ld % EPC == 0 && al(a.dst) && al(a.src)) ? 1 : 0;
    const long items = a.rows * (g.vec ? a.C / EPC : a.C);
    const long want = (items + (long)kThreads * kItemsPerThread - 1) / ((long)kThreads * kItemsPerThread);
    blocks += (unsigned)std::min<long>(std::max<long>(want, 1), kMaxBlocksPerSeg);
    tb.blk_end[tb.n] = blocks;
    ++tb.n;
    bytes += 3.0 * (double)a.rows * a.C * sizeof(T);
  }
  if (tb.n == 0) return 0;
  AfProfScope prof(AF_K_CONTROL_ADD, s, 0.0, bytes);
  hipLaunchKernelGGL((control_add_kernel<T>), dim3(blocks), dim3(kThreads), 0, s, tb);
  HIP_CHECK_RET(hipGetLastError());
  g_af_control_add_launches.fetch_add(1, std::memory_order_relaxed);
  return 0;
}

#define AF_CONTROL_INST(T) template int af_launch_control_add<T>(const AfControlSeg*, int, hipStream_t);
AF_CONTROL_INST(bf16)
AF_CONTROL_INST(f16)
AF_CONTROL_INST(float)
