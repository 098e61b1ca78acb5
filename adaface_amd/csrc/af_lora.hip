// adaface_amd — LoRA adapters (Hu et al., "LoRA: Low-Rank Adaptation of Large Language Models", ICLR 2022) merged into a conv /
// linear weight WHILE it is repacked: what repack_weight_kernel (af_elementwise.hip) does for the base weight alone, with
//
//   v        = src[o][c][tap] + sum over adapters a ascending ( s_a * acc_a )          fp32, then rounded ONCE to T
//   acc_a    = sum over r ascending ( up_a[o][r] * down_a[r][c * kk + tap] )           fmaf chain from +0
//   dst[(row_off + perm(o)) * ldw + tap * cin_pad + c] = from_f32<T>(v)                columns cin <= c < cin_pad: zero
//
// so no fp32 copy of the merged matrix exists anywhere.  up is lora_up.weight [rows][r] (trailing dims 1), down is
// lora_down.weight flattened in its own order [r][cin][ks][ks]: its flat column j = c * kk + tap is also the base weight's, so
// the kernel works on the [rows][K = cin * kk] view of both and only the store knows about taps and padding.
//
// One workgroup (256 threads) per 64 x 64 tile of that view, a 4 x 4 register micro-tile per thread.  Per adapter the rank is
// walked in chunks of 32: up[64 rows][32] (stored k-major, pitch 68 floats) and down[32][64 columns] go through LDS, a thread
// reads one float4 of each per k (the up read is a broadcast within a 16-lane row group, the down read covers 256 contiguous
// bytes: conflict-free) for 16 fmaf.  A rank that is no multiple of the chunk, rows and columns beyond the matrix are staged as
// zeros: fmaf(0, 0, acc) = acc, so the tail adds nothing and the order of an element's operations does not depend on the
// tile.  Vector fp32 FMAs, not MFMA: the products and partial sums are exact fp32 operations in the stated order (file-wide
// contract(off) and explicit fmaf).  With zero adapters v = src: the bits of repack_weight_kernel.
// No atomics, no inter-workgroup traffic; every destination element is written by exactly one thread (the padding columns by
// the workgroups of the first column tile).
#include "../../include/adaface_hip.h"
#include "af_common.h"
#include "af_kernels.h"

#pragma clang fp contract(off)

namespace lora {

constexpr int TM = 64;            // rows of a tile
constexpr int TN = 64;            // columns (c * kk + tap) of a tile
constexpr int KC = 32;            // ranks per LDS chunk
constexpr int UP_LD = TM + 4;     // pitch of the k-major up tile: float4 reads stay 16-byte aligned, staging writes spread over 8 banks

struct Args {
  const float* src;
  const float* up[AF_LORA_MAX_ADAPTERS];
  const float* down[AF_LORA_MAX_ADAPTERS];
  int rank[AF_LORA_MAX_ADAPTERS];
  float scale[AF_LORA_MAX_ADAPTERS];
  int n;
  int rows, cin, cin_pad, kk, ldw, row_off, perm;
  int K;                          // cin * kk
};

template <typename T> __global__ __launch_bounds__(256) void lora_repack_kernel(const Args a, T* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) float up_s[KC * UP_LD];
  __shared__ __attribute__((aligned(16))) float dn_s[KC * TN];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int row0 = blockIdx.y * TM, col0 = blockIdx.x * TN;
  const int o0 = row0 + ty * 4, j0 = col0 + tx * 4;

  float v[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
      v[m][n] = (o0 + m < a.rows && j0 + n < a.K) ? a.src[(long)(o0 + m) * a.K + j0 + n] : 0.f;

  for (int ad = 0; ad < a.n; ++ad) {      // (block-uniform: the barriers below are reached by every thread)
    const float* __restrict__ up = a.up[ad];
    const float* __restrict__ down = a.down[ad];
    const int r = a.rank[ad];
    float acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[m][n] = 0.f;
    for (int k0 = 0; k0 < r; k0 += KC) {
      __syncthreads();                    // the previous chunk has been consumed
#pragma unroll
      for (int i = 0; i < TM * KC / 256; ++i) {      // up: k fastest, as it lies in memory
        const int idx = tid + 256 * i, k = idx % KC, row = idx / KC;
        const bool ok = row0 + row < a.rows && k0 + k < r;
        up_s[k * UP_LD + row] = ok ? up[(long)(row0 + row) * r + k0 + k] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < KC * TN / 256; ++i) {      // down: column fastest
        const int idx = tid + 256 * i, col = idx % TN, k = idx / TN;
        const bool ok = col0 + col < a.K && k0 + k < r;
        dn_s[k * TN + col] = ok ? down[(long)(k0 + k) * a.K + col0 + col] : 0.f;
      }
      __syncthreads();
#pragma unroll 8
      for (int k = 0; k < KC; ++k) {
        const float4 u = *reinterpret_cast<const float4*>(&up_s[k * UP_LD + ty * 4]);
        const float4 d = *reinterpret_cast<const float4*>(&dn_s[k * TN + tx * 4]);
        const float uu[4] = {u.x, u.y, u.z, u.w}, dd[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n) acc[m][n] = fmaf(uu[m], dd[n], acc[m][n]);
      }
    }
    const float s = a.scale[ad];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) v[m][n] = fmaf(s, acc[m][n], v[m][n]);
  }

  const int half = a.rows >> 1;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int o = o0 + m;
    if (o >= a.rows) continue;
    const int rr = a.perm ? geglu_perm(o, half) : o;
    T* drow = dst + (long)(a.row_off + rr) * a.ldw;
    // a 1 x 1 weight keeps the four columns of the micro-tile adjacent: one 8- / 16-byte store where it is whole and aligned
    if (a.kk == 1 && j0 + 3 < a.K && ((uintptr_t)(drow + j0) & (4 * sizeof(T) - 1)) == 0) {
      Quad<T> q;
#pragma unroll
      for (int n = 0; n < 4; ++n) q.e[n] = from_f32<T>(v[m][n]);
      *reinterpret_cast<Quad<T>*>(drow + j0) = q;
      continue;
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int j = j0 + n;
      if (j >= a.K) continue;
      const int c = j / a.kk, tap = j - c * a.kk;
      drow[tap * a.cin_pad + c] = from_f32<T>(v[m][n]);
    }
  }

  // the padding columns of this tile's rows, once per row tile
  const int npad = a.cin_pad - a.cin;
  if (blockIdx.x == 0 && npad > 0) {
    const int per_row = a.kk * npad;
    for (int i = tid; i < TM * per_row; i += 256) {
      const int row = i / per_row, rem = i - row * per_row, tap = rem / npad, c = a.cin + rem - tap * npad;
      const int o = row0 + row;
      if (o >= a.rows) break;             // (rows ascend with i)
      const int rr = a.perm ? geglu_perm(o, half) : o;
      dst[(long)(a.row_off + rr) * a.ldw + tap * a.cin_pad + c] = from_f32<T>(0.f);
    }
  }
}

}  // namespace lora

template <typename T>
int af_launch_lora_repack(const float* src, void* dst, int rows, int cin, int cin_pad, int ks, int ldw, int row_off, int perm,
                          int n_adapters, const float* const* up, const float* const* down, const int* ranks,
                          const float* scales, hipStream_t s) {
  if (!src || !dst || rows <= 0 || cin <= 0 || cin_pad < cin || ks <= 0 || row_off < 0) { af_set_error_msg("lora repack: bad argument"); return -1; }
  const long kk = (long)ks * ks;
  if (kk * cin_pad > ldw || kk * cin > 0x7fffffffL) { af_set_error_msg("lora repack: %ld taps of %d columns do not fit a row of %d", kk, cin_pad, ldw); return -1; }
  if (perm && rows % 32 != 0) { af_set_error_msg("lora repack: the GEGLU row order needs rows %% 32 == 0 (got %d)", rows); return -1; }
  if (n_adapters < 0 || n_adapters > AF_LORA_MAX_ADAPTERS) { af_set_error_msg("lora repack: %d adapters (at most %d)", n_adapters, AF_LORA_MAX_ADAPTERS); return -1; }
  if (n_adapters > 0 && (!up || !down || !ranks || !scales)) { af_set_error_msg("lora repack: null adapter arrays"); return -1; }
  lora::Args a{};
  a.src = src;
  a.n = n_adapters;
  for (int i = 0; i < n_adapters; ++i) {
    if (!up[i] || !down[i]) { af_set_error_msg("lora repack: adapter %d has a null matrix", i); return -1; }
    if (ranks[i] < 1 || ranks[i] > AF_LORA_MAX_RANK) { af_set_error_msg("lora repack: adapter %d has rank %d (1 .. %d)", i, ranks[i], AF_LORA_MAX_RANK); return -1; }
    if (!(scales[i] == scales[i]) || scales[i] - scales[i] != 0.f) { af_set_error_msg("lora repack: adapter %d has a scale that is not finite", i); return -1; }
    a.up[i] = up[i]; a.down[i] = down[i]; a.rank[i] = ranks[i]; a.scale[i] = scales[i];
  }
  a.rows = rows; a.cin = cin; a.cin_pad = cin_pad; a.kk = (int)kk; a.ldw = ldw; a.row_off = row_off; a.perm = perm;
  a.K = (int)(kk * cin);
  const dim3 grid((unsigned)((a.K + lora::TN - 1) / lora::TN), (unsigned)((rows + lora::TM - 1) / lora::TM));
  if (grid.y > 65535u) { af_set_error_msg("lora repack: %d rows are too many for one launch", rows); return -1; }
  hipLaunchKernelGGL((lora::lora_repack_kernel<T>), grid, dim3(256), 0, s, a, reinterpret_cast<T*>(dst));
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
template int af_launch_lora_repack<bf16>(const float*, void*, int, int, int, int, int, int, int, int, const float* const*, const float* const*, const int*, const float*, hipStream_t);
template int af_launch_lora_repack<float>(const float*, void*, int, int, int, int, int, int, int, int, const float* const*, const float* const*, const int*, const float*, hipStream_t);
template int af_launch_lora_repack<f16>(const float*, void*, int, int, int, int, int, int, int, int, const float* const*, const float* const*, const int*, const float*, hipStream_t);
