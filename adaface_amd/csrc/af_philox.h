// Counter-based noise: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel Random Numbers: As Easy as 1, 2, 3", SC'11) and the
// bits -> normals map, shared by the host (af_philox4x32_10) and the device (af_philox.hip).
//
// THE KEYING CONTRACT.  A sample's noise is a pure function of (seed, sample id, stream, step, element) -- never of the rank,
// the batch position or the launch that produced it:
//   key     = (seed lo32, seed hi32)
//   counter = (g, (step << 8) | stream, id lo32, id hi32)
//   id      = the sample's GLOBAL index (int64 >= 0)
//   g       = the index of the group of four consecutive elements inside the sample: element e -> group e / 4, lane e % 4
//             (a sample length that is no multiple of 4 uses the leading lanes of its last group)
//   step < 2^24, stream < 256.  Streams: 0 = start code x_T, 1 = sampler step noise, 2 = q_sample noise of the inpainting blend.
//
// BITS -> NORMALS (Box-Muller, fp32).  For the pairs (r0, r1) and (r2, r3):
//   u = ((r_even >> 9) + 0.5) 2^-23  in (0, 1),   v = (r_odd >> 8) 2^-24  in [0, 1),   both exact in fp32
//   rho = sqrtf(-2 logf(u)),  lanes 0, 1 = rho cospi(2 v), rho sinpi(2 v);  lanes 2, 3 from the second pair
//   |z| <= sqrt(48 ln 2) ~ 5.77.  The accurate logf / sincospif, not the fast intrinsics.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AF_PHILOX_HD __host__ __device__ __forceinline__
#else
#define AF_PHILOX_HD inline
#endif

enum { AF_NOISE_STREAM_XT = 0, AF_NOISE_STREAM_STEP = 1, AF_NOISE_STREAM_QSAMPLE = 2 };

AF_PHILOX_HD uint32_t af_philox_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

// ten rounds; the key is bumped by the Weyl constants between rounds (nine times)
AF_PHILOX_HD void af_philox4x32_10_bits(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                        uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = af_philox_mulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = af_philox_mulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four words of group g of sample id (the contract above)
AF_PHILOX_HD void af_philox_group_bits(uint64_t seed, uint64_t id, uint32_t stream_id, uint32_t step, uint32_t g, uint32_t out[4]) {
  af_philox4x32_10_bits(g, (step << 8) | stream_id, (uint32_t)id, (uint32_t)(id >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), out);
}

#if defined(__HIPCC__)
// one Box-Muller pair.  2 (r_even >> 9) + 1 < 2^24 and r_odd >> 8 < 2^24 convert exactly, and so do the products with a
// power of two; z0 and z1 are each ONE rounded product, so a caller that uses one of them gets the bits of a caller that
// uses both.
__device__ __forceinline__ void af_philox_normal_pair(uint32_t r_even, uint32_t r_odd, float& z0, float& z1) {
  const float u = (float)(2u * (r_even >> 9) + 1u) * 0x1p-24f;
  const float v2 = (float)(r_odd >> 8) * 0x1p-23f;   // 2 v
  const float rho = sqrtf(-2.0f * logf(u));
  float s, c;
  sincospif(v2, &s, &c);
  z0 = rho * c;
  z1 = rho * s;
}
__device__ __forceinline__ void af_philox_normal4(uint64_t seed, uint64_t id, uint32_t stream_id, uint32_t step, uint32_t g,
                                                  float z[4]) {
  uint32_t r[4];
  af_philox_group_bits(seed, id, stream_id, step, g, r);
  af_philox_normal_pair(r[0], r[1], z[0], z[1]);
  af_philox_normal_pair(r[2], r[3], z[2], z[3]);
}
// lane e % 4 of group e / 4 alone: the same bits as that lane of af_philox_normal4
__device__ __forceinline__ float af_philox_normal1(uint64_t seed, uint64_t id, uint32_t stream_id, uint32_t step, uint64_t e) {
  uint32_t r[4];
  af_philox_group_bits(seed, id, stream_id, step, (uint32_t)(e >> 2), r);
  const bool second = (e & 2) != 0;
  float z0, z1;
  af_philox_normal_pair(second ? r[2] : r[0], second ? r[3] : r[1], z0, z1);
  return (e & 1) ? z1 : z0;
}
#endif
