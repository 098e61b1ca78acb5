// adaface_amd — device primitives shared by the kernel files (af_conv_gemm.hip with af_conv_gemm_pp_body.h, af_conv_s8.hip,
// af_xattn_fused.hip, af_attention.hip, af_guidance.hip): the asm / builtin wrappers whose exact form was learned the hard way, once each.
// Device code only: nothing on the host side includes this.  What looks alike but is not the same stays with its kernel
// (ring::mma, the two max3f, xhalf_max / xgroup_max, lds_off, tile_coords, the site-specific "+v" pins).
#pragma once
#include "af_common.h"

#include <type_traits>

// HIP's uint4 / uint2 are structs: asm operands (and the raw buffer load / store builtins) must be vectors
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

// Buffer resource over `ptr` (wave-uniform base, 32-bit per-lane byte offsets, raw addressing).  Lanes that must read zero
// (image padding, rows beyond M) get voffset 0xFFFFFFFF: the hardware range check against num_records returns 0 for them
// and drops their stores, so a gather needs neither branches nor 64-bit address arithmetic.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* ptr, int num_records = (int)0xFFFFFFF0u) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(ptr), 0, num_records, 0x00020000);
}

// LDS-DMA: 16 bytes per lane from a buffer resource straight into LDS at (wave-uniform base) + lane*16.
// (The builtin only exists in the device pass; the host pass of a translation unit must not see it, or clang
// silently drops the kernel's host stub.)
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t rs, char* lds_base, unsigned voffset, unsigned soffset) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds_base, 16, voffset, soffset,
                                           0, 0);
#endif
}

// LDS reads with the constant part of the address in the instruction's immediate offset (no VALU add per read)
template <int OFF = 0> __device__ __forceinline__ u32x4 lds_read128(unsigned addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
template <int OFF = 0> __device__ __forceinline__ u32x2 lds_read_tr64(unsigned addr) {
  u32x2 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}

// Counted waits.  vmcnt counts LDS-DMA pieces and vector-memory loads in issue order; LDS reads return in order too.
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void wait_lgkm() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); }
// ... naming the registers the wait covers ("+v"): a data dependency, so hipcc cannot schedule a consumer of them (an MFMA
// on fragments just read) above the wait.  V = u32x4 / u32x2
template <int N, typename V> __device__ __forceinline__ void wait_lgkm(V& a) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(N) : "memory");
}
template <int N, typename V> __device__ __forceinline__ void wait_lgkm(V& a, V& b) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N) : "memory");
}
template <int N, typename V> __device__ __forceinline__ void wait_lgkm(V& a, V& b, V& c, V& d) {   // (one s_waitcnt for two blocks)
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N) : "memory");
}
// ... between scheduling fences, where no register can be named: hipcc hoists register-only MFMAs over a bare asm wait
template <int N> __device__ __forceinline__ void wait_lgkm_fenced() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// f(std::integral_constant<int, I>{}) for I .. N - 1: a loop whose index is a constant expression in the body
template <int I, int N, typename F> __device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// one v_mfma_f32_16x16x32_bf16 on 16-byte fragments
__device__ __forceinline__ f32x4 mma16(const u32x4& a, const u32x4& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// Sum over the 64 lanes of a wave, xor butterfly: fp32 addition commutes, so every lane ends with the same bits, and they
// depend on the 64 values and their lanes alone.  All lanes of the wave must call it.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 1; off < AF_WAVE; off <<= 1) v += __shfl_xor(v, off, AF_WAVE);
  return v;
}

// LayerNorm (mu, rstd) of a row from its sum and sum of squares.  ln_finalize_kernel and every consumer that finalises its
// own rows (rowpanel_kernel, gemm_m128_kernel, xattn_fused_kernel) do this arithmetic on partial sums added in the same
// order.  That does NOT make a row-resident consumer's stored output bit-identical to the ping-pong kernel's on finalised
// statistics: hipcc contracts the variance per kernel -- fma(s2, inv_count, -fl(mu * mu)) in ln_finalize_kernel and
// gemm_m128_kernel, fma(-mu, mu, fl(s2 * inv_count)) in rowpanel_kernel (the disassembly in front of v_rsq_f32) -- so rstd
// can differ in its last bits, and tests/test_ln_fold_gpu.py counts about 1e-5 of the outputs differing between the two
// (408 of 3.1e7 on [16384, 640] -> 1920), each inside its derived bound.  (The summation loops stay at their sites: as part
// of a shared function they changed the code of seven kernels.)
__device__ __forceinline__ float2 ln_mu_rstd(float s1, float s2, float inv_count, float eps) {
  const float mu = s1 * inv_count;
  const float var = fmaxf(s2 * inv_count - mu * mu, 0.f);
  return float2{mu, __builtin_amdgcn_rsqf(var + eps)};
}
