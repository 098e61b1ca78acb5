// Body of xs::xattn_short_kernel / xs::xattn_short_conv_kernel (af_attention.hip), included INSIDE the two kernel functions.
// Expects the compile-time constants DH and CONV (false = plain, true = subject-token conv attention), the kernel parameters p, vt,
// bpw and a ConvCols cv in scope.  (A textual include and not a __forceinline__ function template, as af_conv_gemm_pp_body.h:
// the function form was built and changed the register allocation of the plain kernels; this form leaves xattn_short_kernel<40>
// and <80> bit-identical to the kernels without the conv variant.)  No include guard: it is included once per kernel.
  using C = Cfg<DH>;
  typedef bf16 T;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int head = blockIdx.y * 4 + wave, b = blockIdx.z;
  if (head >= p.H) return;                                          // (wave-uniform; no barrier in this kernel)
  const T* Q = reinterpret_cast<const T*>(p.q) + (long)b * p.bsq + head * DH;
  const T* K = reinterpret_cast<const T*>(p.k) + (long)b * p.bsk + head * DH;
  T* O = reinterpret_cast<T*>(p.o) + (long)b * p.bso + head * DH;
  const float sl2 = p.scale * 1.44269504088896340736f;

  // ---- resident operand fragments ----
  uint4 kf[NKB][C::KS];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
    for (int s = 0; s < C::KS; ++s) {
      const int key = 32 * kb + l31, d0 = 16 * s + 8 * h;
      Vec16<T> v;
      v.u = make_uint4(0, 0, 0, 0);
      if (key < p.Nk && d0 < DH) v.u = *reinterpret_cast<const uint4*>(K + (long)key * p.ldk + d0);
      // K and Q go into the MFMA as loaded (round 4: scale * log2(e) used to ride on these fragments, a second bf16 rounding
      // of K); the factor enters in the fp32 fma in front of the exponential: softmax is exp2(s * sl2 - m * sl2)
      kf[kb][s] = v.u;
    }
  uint4 vf[C::DB][C::VSTEPS];
  {
    const uint4* vp = reinterpret_cast<const uint4*>(vt + ((long)b * p.H + head) * C::PACK_ELEMS_PER_HEAD);
#pragma unroll
    for (int db = 0; db < C::DB; ++db)
#pragma unroll
      for (int ks = 0; ks < C::VSTEPS; ++ks) vf[db][ks] = vp[((db * C::VSTEPS + ks) * 2 + h) * 32 + l31];
  }
  auto load_q = [&](int blk, uint4 (&qf)[C::KS]) {
    const int q = blk * 32 + l31;
#pragma unroll
    for (int s = 0; s < C::KS; ++s) {
      const int d0 = 16 * s + 8 * h;
      qf[s] = make_uint4(0, 0, 0, 0);
      if (q < p.Nq && d0 < DH) qf[s] = *reinterpret_cast<const uint4*>(Q + (long)q * p.ldq + d0);
    }
  };
  const int nblk = (p.Nq + 31) / 32;
  const int blk0 = blockIdx.x * bpw, blk1 = blk0 + bpw < nblk ? blk0 + bpw : nblk;
  if (blk0 >= nblk) return;
  // conv variant: which subject token a key slot holds is decoded ONCE per wave into a wave-private LDS table, one word per
  // slot: (offset of A_g(y - dy, x - dx) relative to the lane's own pixel) << 5 | 4 (dy + 1) + (dx + 1), the bit of the lane's
  // inside-the-map mask that the shift (dy, dx) tests; a slot outside the subject rows tests bit 16, which is never set.
  // Accumulator register r of key block kb is slot 32 kb + acc_row(r, h): a lane reads its entry with one ds_read.
  [[maybe_unused]] __shared__ int ctab[CONV ? 4 : 1][CONV ? SMAX : 1];
  [[maybe_unused]] const float* cmap = nullptr;
  [[maybe_unused]] unsigned czero = 0;
  if constexpr (CONV) {
    const int ks = cv.ks, nt = ks * ks, p0 = ks == 2 ? 0 : 1;
    cmap = cv.amap + ((long)b * p.H + head) * p.Nq;
    czero = (unsigned)(cv.zero - ((long)b * p.H + head) * p.Nq);
    for (int slot = lane; slot < SMAX; slot += 64) {
      const int rel = slot - cv.tok0;
      const bool in = (unsigned)rel < (unsigned)cv.nsub;
      const int g = in ? rel / nt : 0, j = in ? rel - g * nt : 0;
      const int dy = j / ks - p0, dx = j % ks - p0;
      ctab[wave][slot] = (g * (int)cv.gs - dy * cv.Ww - dx) * 32 + (in ? 4 * (dy + 1) + (dx + 1) : 16);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // (wave-private table, LDS operations of a wave complete in order)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  // one block of 32 queries (fragments qraw, as loaded): S^T, softmax, O^T, store
  auto body = [&](const uint4 (&qf)[C::KS], int blk) {
    // ---- conv columns of this lane's query, gathered ahead of the MFMAs that hide their latency ----
    [[maybe_unused]] float cva[NKB][16];
    if constexpr (CONV) {
      const int qq = blk * 32 + l31;
      const int y = qq / cv.Ww, x = qq - y * cv.Ww;
      // bit 4 (dy + 1) + (dx + 1) of okm: pixel (y - dy, x - dx) lies inside the map (dy, dx in -1 .. 2); bits 16.. stay 0
      unsigned xm = 0, okm = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) xm |= ((unsigned)(x - (i - 1)) < (unsigned)cv.Ww ? 1u : 0u) << i;
#pragma unroll
      for (int i = 0; i < 4; ++i) okm |= ((unsigned)(y - (i - 1)) < (unsigned)cv.Hh ? xm : 0u) << (4 * i);
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        if (32 * kb < cv.tok0 + cv.nsub && 32 * kb + 32 > cv.tok0) {   // (wave-uniform) key blocks without a subject row skip
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int e = ctab[wave][32 * kb + acc_row(r, h)];           // the key this register holds: map offset << 5 | shift bit
            const unsigned ok = __builtin_amdgcn_ubfe(okm, (unsigned)e & 31u, 1u);
            cva[kb][r] = cmap[ok ? (unsigned)(qq + (e >> 5)) : czero];   // (zero fill = the map's zero word: no mask kept, no divergent load)
          }
        }
      }
    }
    // ---- S^T = K Q^T ----
    f32x16 sc[NKB];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[kb][r] = 0.f;
#pragma unroll
      for (int s = 0; s < C::KS; ++s) Mma<T>::step(kf[kb][s], qf[s], sc[kb]);
    }
    if constexpr (CONV) {   // the subject rows := their conv columns
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        if (32 * kb < cv.tok0 + cv.nsub && 32 * kb + 32 > cv.tok0) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if ((unsigned)(32 * kb + acc_row(r, h) - cv.tok0) < (unsigned)cv.nsub) sc[kb][r] = cva[kb][r];
        }
      }
    }
    // ---- exact softmax over the keys < Nk this lane's query column holds (rows split over the two lane halves) ----
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      if (32 * kb + 32 > p.Nk) {       // (wave-uniform) only a partial or empty key block has rows to mask
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (32 * kb + acc_row(r, h) >= p.Nk) sc[kb][r] = -INFINITY;
      }
      // (plain fmaxf: an inline-asm v_max3 reading MFMA results would need its own wait states, see the flash kernels)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[kb][r]);
    }
    mx = xhalf_max(mx);
    const float msl = mx * sl2;
    uint4 pb[NKB][2];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        Vec16<T> v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v.e[j] = from_f32<T>(__builtin_amdgcn_exp2f(fmaf(sc[kb][8 * s2 + j], sl2, -msl)));
        pb[kb][s2] = v.u;
      }
    // ---- O^T = V^T P^T (row DH = the softmax denominator) ----
    f32x16 o[C::DB];
#pragma unroll
    for (int db = 0; db < C::DB; ++db) {
#pragma unroll
      for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) Mma<T>::step(vf[db][2 * kb + s2], pb[kb][s2], o[db]);
    }
    constexpr int rr = DH % 32, ob = DH / 32, oreg = (rr & 3) + 4 * (rr >> 3), oh = (rr >> 2) & 1;
    const float l_tot = __shfl(o[ob][oreg], l31 + 32 * oh, 64);
    const float inv = 1.0f / l_tot;
    const int q = blk * 32 + l31;
#pragma unroll
    for (int db = 0; db < C::DB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int dd = 32 * db + 8 * g + 4 * h;
        if (dd < DH) {
          Quad<T> ov;
#pragma unroll
          for (int e = 0; e < 4; ++e) ov.e[e] = from_f32<T>(o[db][4 * g + e] * inv);
          if (q < p.Nq) ov.store(O + (long)q * p.ldo + dd);
        }
      }
  };
  // Q fragments of THREE blocks in flight (a three-register ring, statically indexed): with one block ahead the wave had
  // ~3 KB of loads outstanding and the launch ran at the memory latency (1.3 TB/s of Q + O traffic), not at its bandwidth
  uint4 q0[C::KS], q1[C::KS], q2[C::KS];
  load_q(blk0, q0);
  load_q(blk0 + 1, q1);           // (blocks past the end load nothing: q >= Nq)
  load_q(blk0 + 2, q2);
  for (int blk = blk0; blk < blk1; blk += 3) {
    body(q0, blk);
    if (blk + 3 < blk1) load_q(blk + 3, q0);
    if (blk + 1 < blk1) {
      body(q1, blk + 1);
      if (blk + 4 < blk1) load_q(blk + 4, q1);
    }
    if (blk + 2 < blk1) {
      body(q2, blk + 2);
      if (blk + 5 < blk1) load_q(blk + 5, q2);
    }
  }
