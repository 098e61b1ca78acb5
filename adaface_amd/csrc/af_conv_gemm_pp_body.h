// Body of the eight-wave ping-pong GEMM kernels, from the tile coordinates to the accumulators: included INSIDE the kernel
// functions of af_conv_gemm.hip (conv_gemm_pp_kernel, ff_geglu_fp8_kernel), which differ in their epilogues only.  Expects
// the compile-time constants BN, GATHER, LNMODE, FP8, SCHED and the kernel parameter `p` in scope; leaves acc, bias_r, the
// LayerNorm operands and the tile / wave coordinates behind for the epilogue.  (A textual include and not a
// __forceinline__ function template: the function form was built and changed the register allocation and instruction
// order of all sixteen conv_gemm_pp_kernel instantiations; this form leaves their code bit-identical,
// profiles/ff8_isa_unchanged_*.txt.)  No include guard: it is included once per kernel.
  static_assert(SCHED == 0 || SCHED == 2, "schedules: 0 phased, 2 merged");
  constexpr bool MG = SCHED == 2;
  constexpr bool FT = GATHER && MG;        // tap masks
  static_assert(MG || !FP8, "fp8 operands exist on the merged schedule only");
  using C = PpCfg<BN>;
  typedef bf16 T;
  static_assert(!FP8 || LNMODE == 0, "fp8 operands: plain epilogue only");
  constexpr unsigned XE = FP8 ? 1u : 2u;   // bytes per operand element
  constexpr int NI = C::NI, MI = C::MI, SLOT = C::SLOT, XBYTES = C::XBYTES;
  // piece split between the two wave groups.  Phased schedules: group 0 all-activation (7 of 8), group 1 the rest and
  // every weight piece.  Merged: every wave stages while it computes, so the gathers are split evenly.
  constexpr int XP0 = MG ? C::XP / 2 : C::XP0;                       // activation pieces of group 0
  constexpr int NX0 = XP0 / 4, NX1 = (C::XP - XP0) / 4;              // ... per wave, group 0 / 1
  constexpr int WP0 = MG ? (C::WP / 8) * 4 : 0;                      // weight pieces of group 0
  constexpr int NW0 = WP0 / 4, NW1 = (C::WP - WP0) / 4;
  constexpr int NP0 = NX0 + NW0, NP1 = NX1 + NW1, NPMAX = NP0 > NP1 ? NP0 : NP1;
  constexpr int NXM = NX0 > NX1 ? NX0 : NX1, NWM = NW0 > NW1 ? NW0 : NW1;
  static_assert(XP0 % 4 == 0 && WP0 % 4 == 0 && NW1 >= 1, "piece split");
  extern __shared__ __attribute__((aligned(1024))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = wid >> 2, wq = wid & 3;
  const int ntm = (p.M + 255) / 256, ntn = p.N / BN;
  int tm, tn;
  tile_coords(blockIdx.x, gridDim.x, ntm, ntn, p.group_m, tm, tn);
  const int m0 = tm * 256, n0 = tn * BN;
  const int zk = blockIdx.z;
  // phase-decomposed upsampled convolution (ConvGemmParams::W_up4): blockIdx.y = output phase, its own padding and weights
  const int ph4 = (GATHER && p.phase4) ? (int)blockIdx.y : 0;
  const int pad_y = (GATHER && p.phase4) ? 1 - (ph4 >> 1) : p.pad, pad_x = (GATHER && p.phase4) ? 1 - (ph4 & 1) : p.pad;

  const __amdgpu_buffer_rsrc_t rs_x = buffer_rsrc(p.src);
  const __amdgpu_buffer_rsrc_t rs_w = buffer_rsrc(p.W);

  // K range of this block (split-K slices)
  const int KT_all = p.K / (FP8 ? 128 : 64);
  const int kt_per = (KT_all + p.splitk - 1) / p.splitk;
  const int kt_begin = zk * kt_per;
  const int KT = min(KT_all, kt_begin + kt_per) - kt_begin;

  // ---- staging state.  Piece q of this wave: group 0: activation piece wq + 4q (q < NP0); group 1: activation
  // piece XP0 + wq + 4q (q < NX1), then weight piece wq + 4(q - NX1).  Lane: row lane>>3 of the piece, LDS slot
  // lane&7, which receives data chunk (lane&7) ^ (row&7).
  const int srow = lane >> 3;
  const unsigned dchunk = (unsigned)((lane & 7) ^ srow);            // data chunk of the 128-byte row this lane fills
  const unsigned lchunk = (FP8 ? (dchunk & 3u) : dchunk) * 16u;     // ... its byte offset inside the 64-channel run
  const int HoWo = p.Ho * p.Wo;
  const unsigned ldcb = (unsigned)p.ldc * XE;
  unsigned x_off[NXM];
  int x_yx[GATHER ? NXM : 1];   // tap masks: validity mask; else (iy0 << 16) | (ix0 & 0xffff): input coordinate of tap (0,0)
  static_for<0, NXM>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    const int piece = g == 0 ? wq + 4 * q : XP0 + wq + 4 * q;
    const int m = m0 + piece * 8 + srow;
    const bool ok = m < p.M && (g == 0 ? q < NX0 : q < NX1);
    const int mm = ok ? m : 0;
    // (b, oy, ox) of the output pixel: shifts when the map sizes are powers of two (every SD-1.5 / VAE level) -- the
    // seven integer divisions per lane cost a few thousand cycles per SIMD at the head of a short-K workgroup
    int b, oy, ox;
    if (p.howo_shift >= 0 && p.wo_shift >= 0) {
      b = mm >> p.howo_shift;
      const int rem = mm & (HoWo - 1);
      oy = rem >> p.wo_shift;
      ox = rem & (p.Wo - 1);
    } else {
      b = mm / HoWo;
      const int rem = mm - b * HoWo;
      oy = rem / p.Wo;
      ox = rem - oy * p.Wo;
    }
    unsigned off = (unsigned)((long)b * p.src_batch_stride * XE) + lchunk;
    if constexpr (GATHER) {
      const int y0 = oy * p.stride - pad_y, x0 = ox * p.stride - pad_x;
      if constexpr (FT) {
        // no upsample: the address of tap (ky, kx) is the tap-(0,0) address plus a wave-uniform delta, and whether the tap
        // falls inside the image is one bit of a mask made here (row bits x column bits) -- the staging phase then spends
        // 4 vector instructions per piece instead of 12, issue slots it competes for with the partner wave's MFMAs
        int vy = 0, vx = 0;
        for (int k = 0; k < p.ks; ++k) {
          vy |= ((unsigned)(y0 + k) < (unsigned)p.Hi ? 1 : 0) << (k * p.ks);
          vx |= ((unsigned)(x0 + k) < (unsigned)p.Wi ? 1 : 0) << k;
        }
        int msk = 0;
        for (int k = 0; k < p.ks; ++k) msk |= ((vy >> (k * p.ks)) & 1) ? (vx << (k * p.ks)) : 0;
        x_yx[q] = ok ? msk : 0;
        off += (unsigned)(y0 * p.Ws + x0) * ldcb;     // (wraps for border pixels; only in-image taps are fetched)
      } else {
        x_yx[q] = ok ? ((y0 << 16) | (x0 & 0xffff)) : (int)0xC0000000;
      }
    } else {
      off += (unsigned)(((oy * p.stride) >> p.up) * p.Ws + ((ox * p.stride) >> p.up)) * ldcb;
      if (!ok) off = 0xFFFFFFFFu;
    }
    x_off[q] = off;
  });
  unsigned w_off[NWM];
#pragma unroll
  for (int q = 0; q < NWM; ++q) {
    const int n = n0 + ((g == 0 ? 0 : WP0) + wq + 4 * q) * 8 + srow;
    w_off[q] = n < p.Wrows ? (unsigned)(((long)ph4 * p.Wrows + n) * p.ldw * XE) + dchunk * 16u : 0xFFFFFFFFu;
  }
  // K order: (channel chunk, tap), the TAP innermost.  The nine taps of a channel chunk re-read the same few input rows back
  // to back, so eight of nine gathers hit the XCD's L2 instead of each tap streaming the whole input slice again (PMC: 225 MB
  // fetched per launch against ~50 MB of input with the tap outermost, the round-1 order).  The weight tile of (tap, chunk)
  // is the 128-byte run at column tap * Cin + c0.  (ks = 1: the plain K walk.)
  // K-walk state of the NEXT tile this wave stages: a plain struct handed around BY VALUE (as by-reference lambda captures
  // mutated inside the merged schedule's compute phase these scalars ended up in scratch, came back as VGPRs, and every
  // LDS-DMA grew a waterfall loop around its scalar offset)
  struct KWalk {
    int ky, kx, c0, ktile;   // filter tap / channel offset / K tile (bf16)
    int u_tap, u_c0;         // fp8, per lane: tap and channel offset of the unit its half of the tile comes from
  };
  KWalk kw;
  kw.ktile = kt_begin;
  kw.u_tap = 0; kw.u_c0 = 0;
  const int taps8 = p.ks * p.ks;
  {
    const int cc = kt_begin / taps8, tap = kt_begin - cc * taps8;
    kw.c0 = cc * 64;
    kw.ky = tap / p.ks;
    kw.kx = tap - kw.ky * p.ks;
  }
  const int adv_q = 2 / taps8, adv_r = 2 - adv_q * taps8;   // fp8: two units further = adv_q chunks + adv_r taps
  if constexpr (FP8) {
    const int u = 2 * kt_begin + (int)(dchunk >> 2);
    const int cc = u / taps8;
    kw.u_tap = u - cc * taps8;
    kw.u_c0 = cc * 64;
  }
  // per-tile staging values, passed BY VALUE from stage_begin to the pieces (as captured variables they are written and
  // read across the "memory"-clobbering fragment-read asm of the merged schedule and end up in scratch)
  struct StageCtx {
    unsigned c0b, k0b;      // scalar byte offsets of the activation channel chunk / the weight K tile
    int live;               // merged schedule: the tile exists (pieces past the K range are issued out of bounds: no
                            // memory traffic, zeros into a slot nobody reads, the vmcnt counts stay fixed)
    int tapbit;             // bf16 tap masks: mask bit of the tap, byte delta of its pixel
    unsigned delta;
    int u_ok;               // fp8 tap masks (per lane): unit inside K, byte delta of its tap + channel offset
    unsigned u_delta;
    int ky, kx, u_tap, u_c0;  // copies for the per-tap bounds arithmetic (phased gathers) / the fp8 unit walk
  };
  auto x_addr = [&](auto qc, const StageCtx& sc) -> unsigned {
    constexpr int q = decltype(qc)::value;
    if constexpr (FP8) {
      if constexpr (GATHER) {
        return ((x_yx[q] >> sc.u_tap) & sc.u_ok) ? x_off[q] + sc.u_delta : 0xFFFFFFFFu;   // (fp8: merged, so tap masks)
      } else {
        return (sc.u_c0 < p.Cin && x_off[q] != 0xFFFFFFFFu) ? x_off[q] + (unsigned)sc.u_c0 : 0xFFFFFFFFu;
      }
    } else if constexpr (FT) {
      return (x_yx[q] & sc.tapbit) ? x_off[q] + sc.delta : 0xFFFFFFFFu;
    } else if constexpr (GATHER) {
      const int iy = (x_yx[q] >> 16) + sc.ky, ix = ((x_yx[q] << 16) >> 16) + sc.kx;
      const bool ok = (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
      const unsigned pix = (unsigned)((iy >> p.up) * p.Ws + (ix >> p.up));
      return ok ? x_off[q] + pix * ldcb : 0xFFFFFFFFu;
    } else {
      return x_off[q];
    }
  };
  // staging of one K tile = stage_begin (wave-uniform / per-lane tap state), one stage_piece per LDS-DMA piece, stage_end
  // (advance to the next tile).  The phased schedule runs the three back to back (stage); the merged one spreads the
  // pieces over the compute phase.
  auto stage_begin = [&](const KWalk& k) -> StageCtx {
    StageCtx sc;
    sc.tapbit = 0; sc.delta = 0u; sc.u_ok = 0; sc.u_delta = 0u;
    sc.ky = k.ky; sc.kx = k.kx; sc.u_tap = k.u_tap; sc.u_c0 = k.u_c0;
    if constexpr (FT) {
      if constexpr (FP8) {
        const int kyl = p.ks == 3 ? (k.u_tap * 11) >> 5 : 0, kxl = p.ks == 3 ? k.u_tap - 3 * kyl : 0;
        sc.u_ok = k.u_c0 < p.Cin ? 1 : 0;
        sc.u_delta = (unsigned)(kyl * p.Ws + kxl) * ldcb + (unsigned)k.u_c0;
      } else {
        sc.tapbit = 1 << (k.ky * p.ks + k.kx);
#ifdef AF_LAB_ABLATE
        if ((p.ablate & 0x100) && (k.ky | k.kx)) sc.tapbit = 0;   // only tap (0,0) fetches activations
#endif
        sc.delta = (unsigned)(k.ky * p.Ws + k.kx) * ldcb;
      }
    }
    sc.c0b = FP8 ? 0u : (unsigned)k.c0 * 2u;
    sc.k0b = FP8 ? (unsigned)k.ktile * 128u : (unsigned)((k.ky * p.ks + k.kx) * p.Cin + k.c0) * 2u;
    sc.live = (!MG || k.ktile < kt_begin + KT) ? 1 : 0;
    return sc;
  };
  auto stage_piece = [&](auto qc, char* base, const StageCtx& sc) {
    constexpr int q = decltype(qc)::value;
    auto fix = [&](unsigned a) -> unsigned { if constexpr (MG) return sc.live ? a : 0xFFFFFFFFu; else return a; };
    if (g == 0) {
      if constexpr (q < NX0) lds_dma16(rs_x, base + (wq + 4 * q) * 1024, fix(x_addr(qc, sc)), sc.c0b);
      else if constexpr (q < NP0) lds_dma16(rs_w, base + XBYTES + (wq + 4 * (q - NX0)) * 1024, fix(w_off[q - NX0]), sc.k0b);
    } else {
      if constexpr (q < NX1) lds_dma16(rs_x, base + (XP0 + wq + 4 * q) * 1024, fix(x_addr(qc, sc)), sc.c0b);
      else if constexpr (q < NP1) lds_dma16(rs_w, base + XBYTES + (WP0 + wq + 4 * (q - NX1)) * 1024, fix(w_off[q - NX1]), sc.k0b);
    }
  };
  auto kw_next = [&](KWalk k) -> KWalk {
    ++k.ktile;
    if constexpr (FP8) {
      k.u_tap += adv_r;
      k.u_c0 += 64 * adv_q;
      if (k.u_tap >= taps8) { k.u_tap -= taps8; k.u_c0 += 64; }
    } else if (++k.kx >= p.ks) {
      k.kx = 0;
      if (++k.ky >= p.ks) { k.ky = 0; k.c0 += 64; }
    }
    return k;
  };
  auto stage = [&](int slot_off) {
    const StageCtx sc = stage_begin(kw);
    char* base = smem + slot_off;
    static_for<0, NPMAX>([&](auto qc) { stage_piece(qc, base, sc); });
    kw = kw_next(kw);
  };

  // ---- fragments: row (lane & 15) of a 16-row block, chunk ((lane >> 4) + 4 u) ^ (row & 7), u = K half ----
  const unsigned lds0 = (unsigned)(__UINTPTR_TYPE__)((__attribute__((address_space(3))) char*)smem);
  const unsigned fch0 = (unsigned)((lane >> 4) ^ (lane & 7)) * 16u;
  const unsigned fch1 = (unsigned)(((lane >> 4) + 4) ^ (lane & 7)) * 16u;
  const unsigned x_base = (unsigned)((wq * 64 + (lane & 15)) * 128);
  const unsigned w_base = (unsigned)(XBYTES + (g * C::HN + (lane & 15)) * 128);

  f32x4 acc[NI][MI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x4 xf[MI][2], wf[NI][2];
#pragma unroll
  for (int i = 0; i < NI; ++i) wf[i][1] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < MI; ++j) xf[j][1] = u32x4{0u, 0u, 0u, 0u};

  // one half of a compute segment: MFMAs of unit UM, the NI + MI fragment reads of unit UR one behind each of the
  // first MFMAs (in-order issue: reads placed after the MFMAs would not overlap them)
  auto half = [&](int slot_off, auto rc, auto mc) {
    constexpr int ur = decltype(rc)::value, um = decltype(mc)::value;
    const unsigned b = lds0 + (unsigned)slot_off + (ur ? fch1 : fch0);
    static_for<0, NI * MI>([&](auto nc) {
      constexpr int n = decltype(nc)::value;
      constexpr int i = n / MI, j = n % MI;
      if constexpr (n < NI) wf[n][ur] = lds_read128<n * 2048>(b + w_base);
      else if constexpr (n < NI + MI) xf[n - NI][ur] = lds_read128<(n - NI) * 2048>(b + x_base);
      acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[i][um]),
                                                          __builtin_bit_cast(bf16x8, xf[j][um]), acc[i][j], 0, 0, 0);
      if constexpr (n < NI + MI) __builtin_amdgcn_sched_barrier(0);
    });
  };
  std::integral_constant<int, 0> U0;
  std::integral_constant<int, 1> U1;

  // bias of this lane's output channels (GEGLU: value and gate rows), fetched now so the main loop hides the latency
  const int cl = 4 * (lane >> 4);
  float4 bias_r[NI];
  auto load_bias = [&]() {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      bias_r[i] = float4{0.f, 0.f, 0.f, 0.f};
      if (p.bias && p.splitk <= 1) bias_r[i] = *reinterpret_cast<const float4*>(p.bias + n0 + g * C::HN + i * 16 + cl);
    }
  };
  if constexpr (!MG) load_bias();   // (merged schedule: 104 fragment registers in the loop; the bias is fetched after it)

  // LayerNorm consumer: column sums of W * gamma for this lane's channels and mu / rstd of its four rows
  float4 ln_cs[LNMODE == 1 ? NI : 1];
  float ln_mu[LNMODE == 1 ? MI : 1], ln_rs[LNMODE == 1 ? MI : 1];
  if constexpr (LNMODE == 1) {
#pragma unroll
    for (int i = 0; i < NI; ++i) ln_cs[i] = *reinterpret_cast<const float4*>(p.ln_colsum + n0 + g * C::HN + i * 16 + cl);
#pragma unroll
    for (int j = 0; j < MI; ++j) {   // (mu, rstd) per row, finalised by ln_finalize_kernel; consumed in the epilogue only
      const int m = m0 + wq * 64 + j * 16 + (lane & 15);
      float2 st = float2{0.f, 0.f};
      if (m < p.M) st = *reinterpret_cast<const float2*>(p.ln_stats + (long)m * 2);
      ln_mu[j] = st.x;
      ln_rs[j] = st.y;
    }
  }

  // ---- merged schedule: fragments and compute phase (bf16 and fp8) ----
  // Order of a tile's 20 (16) MFMAs: weight block outermost, and the LAST weight block's four MFMAs are held back to the
  // head of the next tile's compute phase, where they cover the latency of that tile's first fragment reads (nothing of
  // a tile can be read before the barrier that opens its phase).  They need the previous tile's activation fragments, so
  // those are double-buffered (xa8 / xb8 alternate per tile).  Reads are issued in the order W0 X0 X1 X2 X3 W1 .. W(NI-1):
  // two blocks up front, then one block (two ds_read_b128) behind each MFMA; every MFMA waits with a counted lgkmcnt for
  // exactly the blocks it needs (LDS reads return in order).
  u32x4 w8[MG ? NI : 1][2], xa8[MG ? MI : 1][2], xb8[MG ? MI : 1][2];
  int wsc8[FP8 ? NI : 1];
  int xsc8 = p.x_scale_e8;
  if constexpr (MG && !FP8) {
#pragma unroll
    for (int i = 0; i < NI; ++i) w8[i][0] = w8[i][1] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < MI; ++j) xa8[j][0] = xa8[j][1] = xb8[j][0] = xb8[j][1] = u32x4{0u, 0u, 0u, 0u};
  }
  if constexpr (FP8) {
    // the activation scale as a VGPR made HERE: first used inside the loop, the kernel-argument load behind it would get
    // its s_waitcnt lgkmcnt(0) in front of the first MFMA of every other tile, draining the fragment reads just issued
    asm volatile("" : "+v"(xsc8));
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      w8[i][0] = w8[i][1] = u32x4{0u, 0u, 0u, 0u};
      wsc8[i] = (int)p.w_scale[n0 + g * C::HN + i * 16 + (lane & 15)];
    }
#pragma unroll
    for (int j = 0; j < MI; ++j) xa8[j][0] = xa8[j][1] = xb8[j][0] = xb8[j][1] = u32x4{0u, 0u, 0u, 0u};
  }
  auto mfma8 = [&](f32x4& c, const u32x4 (&wv)[2], const u32x4 (&xv)[2], int wscale) {
    if constexpr (!FP8) {   // bf16: the two K halves of the 64-value tile (chunks q and q + 4)
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wv[0]), __builtin_bit_cast(bf16x8, xv[0]), c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wv[1]), __builtin_bit_cast(bf16x8, xv[1]), c, 0, 0, 0);
      asm volatile("" : "+v"(c));
      return;
    }
    const pp_i32x8 a = __builtin_shufflevector(__builtin_bit_cast(pp_i32x4, wv[0]), __builtin_bit_cast(pp_i32x4, wv[1]), 0, 1, 2, 3, 4, 5, 6, 7);
    const pp_i32x8 b = __builtin_shufflevector(__builtin_bit_cast(pp_i32x4, xv[0]), __builtin_bit_cast(pp_i32x4, xv[1]), 0, 1, 2, 3, 4, 5, 6, 7);
    c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, wscale, 0, xsc8);
    asm volatile("" : "+v"(c));   // a use at this point: hipcc otherwise SINKS the whole tile's MFMAs below the last wait
  };
  // counted wait that hands the guarded fragment block through (a data dependency: the MFMA cannot be hoisted over it)
  auto wait_block = [&](auto nc, u32x4 (&blk)[2]) {
    constexpr int n = decltype(nc)::value;
    wait_lgkm<n>(blk[0], blk[1]);
  };
  // (stage_off: the LDS-DMA pieces of tile t + 2 go out one behind every other MFMA)
  // Timing ablations (a separate lab build with -DAF_LAB_ABLATE, scripts/lab/ablate_conv.sh; results are WRONG): bits
  // 4.. of the ablate knob: 0x10 no LDS-DMA in the loop, 0x20 no fragment reads, 0x40 no MFMAs, 0x100 see above
#ifdef AF_LAB_ABLATE
  const int lab = p.ablate >> 4;
#else
  constexpr int lab = 0;
#endif
  auto cphase8 = [&](int slot_off, u32x4 (&xc)[MG ? MI : 1][2], u32x4 (&xp)[MG ? MI : 1][2], int stage_off,
                     const StageCtx& sc) {
    if constexpr (MG) {
      constexpr int NB = NI + MI;
      char* sbase = smem + stage_off;
      const unsigned b0 = lds0 + (unsigned)slot_off + fch0, b1 = lds0 + (unsigned)slot_off + fch1;
      auto rd_block = [&](auto bc) {
        constexpr int bi = decltype(bc)::value;
        if (lab & 2) return;
        if constexpr (bi == 0) {
          w8[0][0] = lds_read128<0>(b0 + w_base);
          w8[0][1] = lds_read128<0>(b1 + w_base);
        } else if constexpr (bi <= MI) {
          xc[bi - 1][0] = lds_read128<(bi - 1) * 2048>(b0 + x_base);
          xc[bi - 1][1] = lds_read128<(bi - 1) * 2048>(b1 + x_base);
        } else {
          w8[bi - MI][0] = lds_read128<(bi - MI) * 2048>(b0 + w_base);
          w8[bi - MI][1] = lds_read128<(bi - MI) * 2048>(b1 + w_base);
        }
      };
      rd_block(std::integral_constant<int, 0>{});
      rd_block(std::integral_constant<int, 1>{});
      __builtin_amdgcn_sched_barrier(0);
      static_for<0, MI * NI>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        if constexpr (m < MI) {
          if (!(lab & 4)) mfma8(acc[NI - 1][m], w8[NI - 1], xp[m], wsc8[FP8 ? NI - 1 : 0]);   // held back from the previous tile
        } else {
          constexpr int i = (m - MI) / MI, j = (m - MI) % MI;
          constexpr int issued = (2 + m) < NB ? (2 + m) : NB;               // blocks issued before this MFMA
          constexpr int need = i == 0 ? 1 + j : (j == 0 ? MI + i : -1);     // youngest block it reads
          if constexpr (need >= 0) {
            std::integral_constant<int, 2 * (issued - need - 1)> cnt;
            if constexpr (i == 0) wait_block(cnt, xc[j]); else wait_block(cnt, w8[i]);
            if constexpr (i == 0 && j == 0) wait_block(cnt, w8[0]);
          }
          if (!(lab & 4)) mfma8(acc[i][j], w8[i], xc[j], wsc8[FP8 ? i : 0]);
        }
        if constexpr (2 + m < NB) rd_block(std::integral_constant<int, 2 + m>{});
        if constexpr (m >= MI && (m - MI) / 2 < NPMAX) {
          // (the two waves of a SIMD issue their pieces behind alternate MFMAs: group 0 behind the even ones, group 1 odd)
          if (!(lab & 1) && g == ((m - MI) & 1)) stage_piece(std::integral_constant<int, (m - MI) / 2>{}, sbase, sc);
        }
        __builtin_amdgcn_sched_barrier(0);
      });
      static_assert(MI + 2 * (NPMAX - 1) + 1 < MI * NI, "merged schedule: a staging slot behind an MFMA for every piece");
      wait_lgkm_fenced<0>();       // every read of the tile is back (the last weight block included)
    }
  };

  int rd = 0, w0 = SLOT, w1 = 2 * SLOT;       // slots of tiles t, t+1, t+2
  if constexpr (MG) {
    // ---- merged schedule: tiles 0 and 1 in flight (every wave its own pieces), then per tile: own pieces of tile t
    // landed (tile t + 1's stay in flight) -> barrier (tile t complete and visible; everyone done reading tile t - 1) ->
    // compute tile t while staging tile t + 2 into the slot of tile t - 1
    stage(0);
    stage(SLOT);
    auto tile = [&](auto& xc, auto& xp) {
      if (g == 0) wait_vm<NP0>(); else wait_vm<NP1>();
      __builtin_amdgcn_s_barrier();
      // (gathers: tap masks only -- the launcher sends upsampled convolutions to the phased schedule)
      const StageCtx sc = stage_begin(kw);
      cphase8(rd, xc, xp, w1, sc);
      kw = kw_next(kw);
      const int tmp = rd; rd = w0; w0 = w1; w1 = tmp;
    };
    for (int t = 0; t + 1 < KT; t += 2) {   // (pairs: no branch inside the body, so no register shuffles where paths merge)
      tile(xa8, xb8);
      tile(xb8, xa8);
    }
    if (KT & 1) tile(xa8, xb8);
    wait_vm<0>();          // the out-of-range pieces of tiles KT, KT + 1 (zero fill) before the epilogue reuses the LDS
    if (KT & 1) {
#pragma unroll
      for (int j = 0; j < MI; ++j) mfma8(acc[NI - 1][j], w8[NI - 1], xa8[j], wsc8[FP8 ? NI - 1 : 0]);
    } else {
#pragma unroll
      for (int j = 0; j < MI; ++j) mfma8(acc[NI - 1][j], w8[NI - 1], xb8[j], wsc8[FP8 ? NI - 1 : 0]);
    }
    __builtin_amdgcn_s_barrier();
  } else {
    // ---- phased schedule, prologue: tile 0 (group 1 also tile 1) in flight; group 1's part of tile 0 landed ----
    auto wait_keep1 = [&]() { if (g == 0) wait_vm<NP0>(); else wait_vm<NP1>(); };
    stage(0);
    if (g == 1) {
      if (KT > 1) { stage(SLOT); wait_keep1(); } else wait_vm<0>();
    }
    __builtin_amdgcn_s_barrier();
    if (g == 1) __builtin_amdgcn_s_barrier();   // group 1 runs one interval behind
    auto dphase = [&](int t) {
      if (g == 0) {
        if (t + 1 < KT) { stage(w0); wait_keep1(); } else wait_vm<0>();   // own part of tile t landed
      } else {
        if (t + 2 < KT) stage(w1);
      }
      __builtin_amdgcn_s_barrier();
    };
    auto cend = [&](int t) {
      if (g == 1) { if (t + 2 < KT) wait_keep1(); else wait_vm<0>(); }    // own part of tile t+1 landed
      __builtin_amdgcn_s_barrier();
      const int tmp = rd; rd = w0; w0 = w1; w1 = tmp;
    };
    for (int t = 0; t < KT; ++t) {
      // ---------------- D(t) ----------------
      dphase(t);
      // ---------------- C(t) ----------------
      __builtin_amdgcn_s_setprio(1);
      half(rd, U0, U1);      // (t == 0: MFMAs on the zeroed fragments of "unit -1")
      wait_lgkm_fenced<0>();
      half(rd, U1, U0);
      wait_lgkm_fenced<0>();       // every read of tile t is back: the barrier below releases its slot
      __builtin_amdgcn_s_setprio(0);
      cend(t);
    }
    // trailing half tile (unit 2 KT - 1), registers only
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < MI; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[i][1]),
                                                            __builtin_bit_cast(bf16x8, xf[j][1]), acc[i][j], 0, 0, 0);
    if (g == 0) __builtin_amdgcn_s_barrier();
  }
  if constexpr (MG) load_bias();

