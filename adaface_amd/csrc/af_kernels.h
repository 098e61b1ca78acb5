// Internal launcher declarations (one template per storage type T = bf16 | float | f16).
#pragma once
#include "af_common.h"

// The plan of a conv / linear launch: kernel, tile, K slices (AfGemmPlan, af_common.h).  have_ws = false: the launch gets no
// workspace for K slabs.  A caller that needs to know what will run -- fp8 or not, row-panel or not, how much workspace -- asks
// here and hands the plan to the launcher; the launcher plans itself when it gets none.
AfGemmPlan af_plan_conv_gemm(const ConvGemmParams& p, int batch, AfStorage st, bool have_ws = true);
template <typename T>
int af_launch_conv_gemm(const ConvGemmParams& p, int batch, hipStream_t stream, const AfGemmPlan* plan = nullptr,
                        void* ws = nullptr);
// The plan of an attention launch (af_attention.hip): which kernel runs.  af_launch_attention follows it and af_attn_plan_query
// reports it, so a test knows on the CPU which kernel a shape, pitch and flag set reaches.  The values are part of that result.
enum AfAttnKernel {
  AF_ATK_REFUSED = 0,    // a head dim outside {8, 16, 32, 40, 64, 80, 128, 160}, a q / k / v pitch that is no whole number of
                         // 16-byte chunks, an output pitch % 4, no key: the launcher fails, nothing runs
  AF_ATK_FLASH = 1,      // attn_kernel<T, DH>: four waves, K / V staged through registers
  AF_ATK_FLASH_W4 = 2,   // attn_kernel_w4<bf16, 40>: the same body capped at 128 VGPRs (bf16 dh 40 without the ring kernel)
  AF_ATK_RING40 = 3,     // ring::attn_ring40_kernel: eight waves, LDS-DMA staging (bf16 dh 40, knob attn_ring bit 0, not causal)
  AF_ATK_RING80 = 4,     // ring::attn_ring80_kernel (bf16 dh 80, attn_ring bit 1, not causal, >= 256 keys or attn_ring bit 2)
  AF_ATK_SHORT = 5,      // xs::xattn_short_kernel (bf16 dh 40 / 80, <= 96 keys, V^T pack present, knob attn_short, no mask, no lse)
  AF_ATK_COUNT = 6
};
AfAttnKernel af_plan_attention(AfStorage st, int dh, int Nk, int ldq, int ldk, int ldv, int ldo, bool causal, bool has_lse,
                               bool has_vt_pack);
// launches per AfAttnKernel since af_gemm_plan_counts_reset, counted where af_launch_attention followed the plan
extern std::atomic<long> g_af_attn_launches[AF_ATK_COUNT];
// Nq <= 0 or B <= 0: nothing to do, 0.  A refused plan: -1 with a message
template <typename T> int af_launch_attention(const AttnParams& p, int B, int dh, hipStream_t stream);
// V packed as the resident MFMA fragments of the short-key cross-attention kernel (bf16; Nk <= 96, dh 40 / 80): elements
// needed (0 = no such kernel for this case) and the pack launch; AttnParams::vt_pack then selects the kernel
template <typename T> long af_attn_short_pack_elems(int B, int H, int dh, int Nk);
template <typename T>
int af_launch_attn_short_pack(const void* v, int ldv, long bsv, int Nk, int H, int dh, int B, void* vt, hipStream_t stream);
// Subject-token conv attention in ONE pass of the short-key kernel (bf16, dh 40 / 80, <= 96 keys with their V^T pack, ks 2..4):
// p covers ALL Nk keys, the groups * ks^2 subject rows at their end (af_set_context's order); amap = the conv maps
// [groups][B][H][Hh * Ww] fp32 + the zero word of af_launch_conv_attn_map.  The predicate is the planner's and the launcher's.
bool af_conv_attn_short_ok(bool is_bf16, int dh, int Nk, bool vt_pack, int ks, int groups);
int af_launch_conv_attn_short(const AttnParams& p, int B, int dh, int ks, int groups, int Hh, int Ww, const float* amap,
                              hipStream_t stream);
extern std::atomic<long> g_af_conv_attn_short_launches;
// ONE launch per cross-attention layer (bf16, C = 320, 8 heads x 40, <= 80 keys; af_xattn_fused.hip): LayerNorm-folded to_q,
// attention over the packed context K / V, to_out + bias + residual, LayerNorm partial sums for the next consumer
struct AfXattnFusedParams {
  const void* x; int ldx; int M; int rows_per_sample;
  const float* ln_stats; int ln_parts_n; float ln_inv_count, ln_eps;   // as ConvGemmParams::ln_stats / ln_parts_n
  const void* wq; int ldwq; const float* q_colsum; const float* q_bias;
  const void* kvpack;                                                  // af_launch_xattn_fused_pack
  const void* wo; int ldwo; const float* o_bias;                       // K-permuted to_out weight (af_launch_xattn_fused_permute_wo)
  void* out; int ldo;
  float* ln_stats_out;                                                 // [4][M][2] or null
  int Nk;
};
bool af_xattn_fused_ok(int M, int rows_per_sample, int C, int H, int dh, int Nk);
long af_xattn_fused_pack_elems(int B, int H, int dh, int Nk);         // bf16 elements of the K / V pack of one layer (0 = no such kernel)
int af_launch_xattn_fused_pack(const void* kv, int ldk, long bsk, int Nk, int B, void* pack, hipStream_t stream);   // K as stored: the kernel applies dh^-1/2 * log2 e in fp32
int af_launch_xattn_fused_permute_wo(const void* w, int ldw, int rows, void* wp, int ldp, hipStream_t stream);
int af_launch_xattn_fused(const AfXattnFusedParams& a, hipStream_t stream);
extern std::atomic<long> g_af_xattn_fused_launches;

// FeedForward scope of the fp8 mode (ff_geglu_fp8_kernel, af_conv_gemm.hip): e4m3 x [M][K] times the e4m3 twin of a GEGLU
// projection -> e4m3 bytes of value * gelu(gate) * out_mul, p.out [M][p.ldo >= N / 2]; rec: optional fp8 calibration record
bool af_ff_geglu_fp8_ok(const ConvGemmParams& p);
int af_launch_ff_geglu_fp8(ConvGemmParams p, float out_mul, unsigned* rec, hipStream_t stream);
extern std::atomic<long> g_af_ff8_launches;

// The plan of a GroupNorm(32) launch (af_norm.hip): which kernels run and how the map is cut.  The launchers follow it and
// af_norm_plan_query reports it, so a test knows on the CPU which kernel a shape reaches.  The values are part of that result.
enum AfGnKernel {
  AF_GNK_REFUSED = 0,    // C the kernels do not take (C % 32, whole 16-byte vectors, C <= 2560): the launcher fails, nothing runs
  AF_GNK_SMALL = 1,      // gn_small_kernel: one launch, a (sample, group) per workgroup held in registers
  AF_GNK_FOLD = 2,       // gn_stats_kernel + gn_apply_kernel, whose blocks combine the <= 64 partial sums themselves
  AF_GNK_FINALIZE = 3    // gn_stats_kernel + gn_finalize_kernel + gn_apply_kernel
};
struct AfGnPlan {
  int kernel;       // AfGnKernel
  int P;            // pixels per chunk (one workgroup of the statistics and the apply pass); 0 on SMALL / REFUSED, as all below
  int nchunk;       // chunks per sample, ceil(HW / P): the last one holds HW - (nchunk - 1) * P pixels
  int npart;        // partial sums per sample the statistics are combined from: nchunk, or the producer convolution's pre_npart
  int wide_stats;   // 1: gn_stats_kernel runs and walks more than 256 vectors per pixel with its one-thread-per-column loop
};
// pre_npart > 0: a producer convolution left that many partial sums per sample and no statistics pass runs.  to_affine: the
// plan of af_launch_groupnorm_fold, which writes no tensor (no small kernel; `kernel` only tells refused from not).
AfGnPlan af_plan_groupnorm(AfStorage st, int B, int HW, int Cn, int pre_npart, bool to_affine = false);
enum AfLnKernel {
  AF_LNK_REFUSED = 0,    // C that is no whole number of 16-byte vectors, or more of them than a wave holds (64 * 5)
  AF_LNK_WAVE_ROW = 1,   // layernorm_kernel: one wave per row, four rows per workgroup
  AF_LNK_ROWGROUP = 2    // layernorm_rowgroup_kernel: 8 (16-bit storage) or 16 (f32) lanes per row
};
struct AfLnPlan {
  int kernel;           // AfLnKernel
  int nv;               // 16-byte vectors a lane holds at most (WAVE_ROW: ceil(vectors / 64), ROWGROUP: vectors / lanes per row)
  int rows_per_block;   // rows of one 256-thread workgroup: 4, or 256 / lanes per row
};
AfLnPlan af_plan_layernorm(AfStorage st, long rows, int Cn);

size_t af_gn_workspace_bytes(int B, int HW);
template <typename T>
int af_launch_groupnorm(const void* x, long x_bs, int ldx, int B, int HW, int Cn, const float* gamma,
                        const float* beta, float eps, int silu, void* y, long y_bs, int ldy, void* workspace,
                        hipStream_t stream, float fp8_mul = 0.f,    // fp8_mul != 0: y is e4m3 bytes of result * fp8_mul
                        const float* pre_partial = nullptr, int pre_npart = 0,    // statistics already summed by the producer
                        unsigned* fp8_rec = nullptr);   // fp8 calibration record {amax bits, n saturated} to update (e4m3 output only)
// GroupNorm reduced to its per-sample affine map ab_out [B][2][Cn] (scale, shift) for a consumer that applies it itself
// (ConvGemmParams::gn_ab): statistics pass (unless pre_partial) + fold, no pass that writes the normalised tensor
template <typename T>
int af_launch_groupnorm_fold(const void* x, long x_bs, int ldx, int B, int HW, int Cn, const float* gamma, const float* beta,
                             float eps, void* workspace, hipStream_t stream, const float* pre_partial, int pre_npart,
                             float* ab_out);
// would a bf16 convolution with these parameters on this plan write GroupNorm partial sums (ConvGemmParams::gn_stats_out)?
bool af_conv_gn_stats_ok(const ConvGemmParams& p, const AfGemmPlan& pl, int cpg);
// the small-map 3x3 convolution kernel (af_conv_s8.hip; planner and launcher only): K slices it runs in (8 x 8 maps: 4,
// 16 x 16 maps: 1), 0 = not taken
int af_conv_s8_slices(const ConvGemmParams& p, int batch);
int af_launch_conv_s8(const ConvGemmParams& p, hipStream_t stream);
template <typename T>
int af_launch_layernorm(const void* x, int ldx, long rows, int Cn, const float* gamma, const float* beta,
                        float eps, void* y, int ldy, hipStream_t stream, float fp8_mul = 0.f, unsigned* fp8_rec = nullptr);

// Token merging in front of the U-Net's self-attention (af_tome.hip; tomesd with sx = sy = 2, use_rand = False).  Storage types
// bf16 and float.  The plan of an H x W map (both even) at `ratio` in [0, 0.75]: Nd = N / 4 dst tokens, Ns = N - Nd src tokens,
// r = min(Ns, int(N * ratio)) of them merged, Np = N - r rows left; -1 with a message for a map or ratio it refuses.
struct AfTomePlan { long Nd, Ns, r, Np; };
int af_tome_plan(int H, int W, double ratio, AfTomePlan* pl);
size_t af_tome_match_ws_bytes(int B, int H, int W);
// x [B][H * W][ldx] -> node_idx / node_max [B][Ns] and map [B][H * W] (values in [0, Np)); normalize: cosine scores.  Launches:
// reciprocal norms (normalize only), match, rank, map.  ws: af_tome_match_ws_bytes bytes
template <typename T>
int af_launch_tome_match(const void* x, int ldx, int B, int H, int W, int C, double ratio, int normalize, int* node_idx,
                         float* node_max, int* map, void* ws, hipStream_t s);
// y [B][Np][ldy]: row j = mean over {i : map[i] = j} of LayerNorm(x_i) (gamma null: of x_i), N <= 16384 tokens per sample
template <typename T>
int af_launch_tome_merge(const void* x, int ldx, const float* gamma, const float* beta, float eps, const int* map, int B, int N,
                         int Np, int C, void* y, int ldy, hipStream_t s);
// y [B][N][ldy] = res + o[map]; ln_stats_out (optional): LayerNorm partial sums [ln_parts][B * N][2] of y's rows
template <typename T>
int af_launch_tome_unmerge_add(const void* o, int ldo, const void* res, int ldr, const int* map, int B, int N, int Np, int C,
                               void* y, int ldy, float* ln_stats_out, int ln_parts, hipStream_t s);

// T-GATE (af_tgate.hip), all three storage types.  t2 [L B][N][ld2] = t1 + src, src [L B][N][lds]; cache (optional)
// [B][N][ldc] = mean over the L legs (1 or 2) of src; ln_stats_out (optional): LayerNorm partial sums [ln_parts][L B N][2] of t2's
// rows.  t2 may be src.  16-byte accesses where every pointer and row stride allows them, element accesses otherwise.
template <typename T>
int af_launch_tgate_add(const void* t1, int ld1, const void* src, int lds, void* t2, int ld2, void* cache, int ldc, int L, int B,
                        int N, int C, float* ln_stats_out, int ln_parts, hipStream_t s);

// ControlNet residual injection (af_controlnet.hip), all three storage types: ONE launch applies up to
// AF_CONTROL_MAX_SEGMENTS segments dst[r][0 .. C) = round(dst[r][c] + round32(scale * src[r][c])), r < rows -- dst rows ld >= C
// elements apart (a channel range of a concatenation buffer), src dense.  Product and sum are separate fp32 roundings (no fma).
// 16-byte accesses per segment where its pointers and row stride allow them, element accesses otherwise.  Nothing outside the
// addressed channel ranges is read or written.  A refused argument: -1 with a message, nothing launched.
enum { AF_CONTROL_MAX_SEGMENTS = 16 };
struct AfControlSeg { void* dst; const void* src; long rows; int C, ld; float scale; };
template <typename T> int af_launch_control_add(const AfControlSeg* segs, int n, hipStream_t s);
extern std::atomic<long> g_af_control_add_launches;   // launches since the library was loaded

// Noising + inpainting blend (af_inpaint.hip): fp32 only, the whole of it behind the ABI's af_noise_blend (which
// checks its arguments on the host and launches ONE kernel); af_noise_blend_launches reads this counter.
extern std::atomic<long> g_af_noise_blend_launches;   // launches since the library was loaded

// LCM / TCD consistency step (af_lcm.hip): fp32 only, the whole of it behind the ABI's af_lcm_step (which checks its
// arguments on the host and launches ONE kernel, instantiated on (CFG, noise source) alone); af_lcm_step_launches reads this.
extern std::atomic<long> g_af_lcm_step_launches;      // launches since the library was loaded

// Self-attention guidance (af_sag.hip).  The attention mass per key of a self-attention site, all three storage
// types: mass [B][N] fp32 = mean over heads of the column sums of softmax(q k^T dh^-0.5); q / k element (b, i, c) at
// p[b bs + i ld + c], c < heads dh.  Two launches: one workgroup per (sample, head) writes that head's column sums into
// part [B][heads][N] (the caller's scratch), a second kernel adds the heads in order; no atomics; N <= 256 (-1 with a message
// above it).  The degrade kernel is fp32 only and sits behind the ABI's af_sag_degrade.  The counters: calls of each since the
// library was loaded.
template <typename T>
int af_launch_sag_mass(const void* q, int ldq, long bsq, const void* k, int ldk, long bsk, float* mass, float* part, int B, int N,
                       int heads, int dh, hipStream_t s);
extern std::atomic<long> g_af_sag_mass_launches;
extern std::atomic<long> g_af_sag_degrade_launches;

// Regional prompts (af_region_attn.hip): the context of a sample is R <= AF_REGION_MAX segments of T keys, a weight
// pyramid says which regions a pixel of a site listens to.  The layout of the pyramid of an H x W map (sides multiples of 8):
// level l (f = 2^l) holds w [Bf][R][N_l] fp32 at float w_off[l] and one word of active-region bits per (sample, 32-query
// block) at word b_off[l]; -1 with a message for a shape it refuses.
enum { AF_REGION_MAX = 8 };
struct AfRegionLayout { long w_off[4], b_off[4], w_floats, b_words; int N[4], nblk[4]; };
int af_region_layout(int Bf, int R, int H, int W, AfRegionLayout* L);
// m [Bf][R][H][W] fp32 >= 0 -> the pyramid and the bits, ONE launch (region_weights_kernel)
int af_launch_region_weights(const float* m, int Bf, int R, int H, int W, float* pyr, unsigned* bits, hipStream_t stream);
// The plan of a regional cross-attention: the ONE decision, which xfmr_cross_attention and af_op_region_attention follow and
// af_region_plan_query reports.  The values are part of that result.
enum AfRegionKernel {
  AF_RGK_REFUSED = 0,    // R outside 1 .. 8, no key, a head dim the attention kernels do not take
  AF_RGK_COMPOSE = 1,    // R launches of af_launch_attention on the key segments + region_combine_kernel (f32, T > 96, other
                         // head dims, knob region_fused = 0)
  AF_RGK_FUSED = 2       // region_attn_kernel<T, DH>: bf16 / fp16, dh in {32, 40, 64, 80, 128, 160}, T <= 96
};
int af_plan_region_attention(AfStorage st, int dh, int T, int R);
// V of the cached [B][R T][..] key list (row pitch ldv, sample stride bsv) as the fused kernel's per-segment V^T fragments:
// elements needed (0 = no fused kernel for this case) and the pack launch
template <typename T> long af_region_pack_elems(int B, int R, int H, int dh, int Tk);
template <typename T>
int af_launch_region_pack(const void* v, int ldv, long bsv, int Tk, int R, int H, int dh, int B, void* vt, hipStream_t stream);
struct AfRegionAttnArgs {
  const void* q; const void* k; void* o; const void* vt;   // k: [B][R T] rows of pitch ldk; vt: af_launch_region_pack
  const float* w; const unsigned* bits;                    // this site's level: w [B][R][Nq], bits [B][ceil(Nq / 32)]
  int ldq, ldk, ldo; long bsq, bsk, bso;                   // elements
  int B, Nq, R, T, heads, dh; float scale;
  int level;                                               // the pyramid level, for the profiler's class only (AF_K_REGION_ATTN + level)
};
template <typename T> int af_launch_region_attention(const AfRegionAttnArgs& a, hipStream_t stream);
// out [B Nq][ldo] = sum_{r : w_r > 0} w_r src[r][B Nq][Cn] (src dense, rs elements between regions), fp32 sum, r ascending
template <typename T>
int af_launch_region_combine(const void* src, long rs, const float* w, void* out, int ldo, int B, int Nq, int Cn, int R,
                             hipStream_t stream);
extern std::atomic<long> g_af_region_attn_launches;   // fused launches since the library was loaded

// FreeU in place on a concatenation buffer [B][H W][ld], pixel rows [h (Ch) | skip (Cs)] (af_freeu.hip).  All three storage
// types.  The plan of one site: the launcher follows it and af_freeu_plan_query reports it.  The values are part of that result.
enum AfFreeuKernel {
  AF_FREEUK_REFUSED = 0,   // a map side < 2, Ch % 16, Cs % 8, a version that is neither 1 nor 2: -1 with a message, nothing runs
  AF_FREEUK_SINGLE = 1,    // freeu_small_kernel: H W <= 256, low-band sums and apply in one launch
  AF_FREEUK_CHUNKED = 2    // freeu_sums_kernel (one partial per 256-pixel chunk) + freeu_apply_kernel
};
struct AfFreeuPlan {
  int kernel;         // AfFreeuKernel
  int launches;       // with backbone and skip both live: 1 / 2, one more (freeu_mean_kernel) for version 2
  int nchunk;         // 256-pixel chunks of a sample's map
  long part_bytes;    // partial sums per sample, [nchunk][7][Cs] fp32 (0 on SINGLE)
};
int af_plan_freeu(int H, int W, int Ch, int Cs, int version, AfFreeuPlan* pl);
size_t af_freeu_ws_bytes(int B, int H, int W, int Ch, int Cs, int version);   // 0 for a refused plan
// backbone / skip false: that half is left alone (b == 1 / s == 1 do the same).  b in [1, 2], s in [0, 1].  ws: af_freeu_ws_bytes
template <typename T>
int af_launch_freeu(void* cat, int ld, int B, int H, int W, int Ch, int Cs, int version, float b, float s, bool backbone,
                    bool skip, void* ws, hipStream_t stream);

// The guidance combine with PAG and rescale (af_guidance.hip, which also holds af_guidance itself).  The plan of one call: the
// launcher follows it and af_guidance_plan_query reports it.  The values are part of that result.
enum AfGuidanceKernel {
  AF_GDK_REFUSED = 0,    // no sample, per_sample < 2 or beyond 2^31, more workgroups than a launch takes: -1 with a message
  AF_GDK_COMBINE = 1,    // rescale off: guidance_combine_kernel, element-wise
  AF_GDK_SINGLE = 2,     // rescale on, per_sample <= 1024: guidance_single_kernel, statistics and apply in one launch
  AF_GDK_CHUNKED = 3     // rescale on: guidance_stats_kernel (one partial per 256-element chunk) + guidance_apply_kernel
};
struct AfGuidancePlan {
  int kernel;         // AfGuidanceKernel
  int launches;       // 1 / 1 / 2
  long nchunk;        // 256-element chunks of a sample
  long part_bytes;    // partials per sample, [nchunk][4] fp32 (CHUNKED only)
};
int af_plan_guidance(long n_samples, long per_sample, bool rescale_on, AfGuidancePlan* pl);

template <typename T>
int af_launch_nchw_to_nhwc(const float* x, void* y, int B, int Cn, int HW, int Cpad, float scale, hipStream_t s);
template <typename T> int af_launch_nhwc_to_nchw(const void* x, float* y, int B, int Cn, int HW, int ld, hipStream_t s);
template <typename T> int af_launch_cast_f32(const float* x, void* y, long n, hipStream_t s);
// fp32 [rows][D] -> T with dst row r taken from src row rowmap[r]
template <typename T>
int af_launch_gather_rows_cast(const float* x, const int* rowmap, void* y, long rows, int D, hipStream_t s);
// subject-token ks x ks conv attention (ldm/util.py:701-879; ks = 2, 3, 4) for B samples whose ks^2 subject keys are rows
// tok0..tok0+ks^2-1 of kv [S][2*H*dh] (K | V): o holds the flash result over the keys in front of the subject tokens (its
// log2-domain log-sum-exp in lse [B][H][N]) and is overwritten by the merged attention output, lse by the merged
// log-sum-exp (several subject strings per sample merge one after the other); sN = scratch [B][H][N][ks^2] floats
template <typename T>
int af_launch_conv_attn(const void* q, int ldq, long bsq, const void* kv, int ldk, long bsk, int tok0, float* sN,
                        float* lse, void* o, int ldo, long bso, int B, int N, int H, int dh, int Hh, int Ww,
                        float scale, int ks, hipStream_t s);
// conv maps of `groups` subject strings whose ks^2 keys are rows tok0 + g * ks^2 + t of k (tap order), for B samples:
// amap[g][b][h][p] = ks^-1.5 * sum_t q[b][p + off_t][h] . k[b][tok0 + g ks^2 + t][h], off_t = (t / ks - P0, t % ks - P0),
// zero outside the Hh x Ww map, fp32 accumulation, WITHOUT the softmax scale (oracle conv_attn_rows' A / scale).  amap holds
// af_conv_attn_map_floats(...) floats: the maps and one zero word behind them (the zero fill of af_launch_conv_attn_short)
inline size_t af_conv_attn_map_floats(int groups, int B, int H, int N) { return (size_t)groups * B * H * N + 1; }
template <typename T>
int af_launch_conv_attn_map(const void* q, int ldq, long bsq, const void* k, int ldk, long bsk, int tok0, int groups,
                            float* amap, int B, int H, int dh, int Hh, int Ww, int ks, hipStream_t s);
template <typename T> int af_launch_cast_to_f32(const void* x, float* y, long n, hipStream_t s);
template <typename T> int af_launch_timestep_embedding(const long long* t, void* y, int B, int dim, hipStream_t s);
template <typename T> int af_launch_silu(const void* x, void* y, long n, hipStream_t s);
// CLIP text tower pieces (encoders/modules.py:179-463; transformers CLIPTextModel)
template <typename T> int af_launch_quick_gelu(const void* x, void* y, long n, hipStream_t s);
template <typename T>
int af_launch_embed_rows(const long long* ids, const void* table, int vocab, int D, float* y, long n, hipStream_t s);
template <typename T>
int af_launch_add_pos_cast(const float* x, const void* pos, int Tn, int D, void* y, long rows, hipStream_t s);
template <typename T> int af_launch_blend2(const void* a, float w0, const void* b, float w1, void* y, long n, hipStream_t s);
template <typename T>
int af_launch_copy_channels(const void* src, int lds_, void* dst, int ldd, int off, int Cn, long npix, hipStream_t s);
int af_launch_ddim_step(const float* x, const float* eps_c, const float* eps_u, const float* noise, long n,
                        float guidance, float a_t, float a_prev, float sqrt_one_minus_at, float sigma_t,
                        float temperature, float* x_prev, float* pred_x0, hipStream_t s);
int af_launch_dpmpp_step(const float* x, const float* eps_c, const float* eps_u, const float* x0_prev, long n, float guidance,
                         float alpha_t, float sigma_t, float c_x, float c_d, float w_cur, float w_prev, float* x_next,
                         float* x0_out, hipStream_t s);
int af_launch_posterior_sample(const float* mom, const float* noise, float scale, float* z, int B, int Cn, long HW,
                               hipStream_t s);
int af_launch_lincomb(float* out, long n, const float* x0, float w0, const float* x1, float w1, const float* x2, float w2,
                      const float* x3, float w3, int mode, hipStream_t s);
template <typename T> int af_launch_softmax_rows(void* x, int ld, int ncols, long rows, hipStream_t s);
template <typename T>
int af_launch_transpose(const void* x, long x_bs, int ldx, void* y, long y_bs, int R, int Cn, int B, hipStream_t s);
// The VAE AttnBlock between its qkv convolution and proj_out (model.py:179-242; defined in af_model.hip, which calls it with
// taps = null; af_op_vae_attention is the other caller): qkv [B][N][3C] of storage type `dtype` (q | k | v per position) ->
//   sc [B][N][N]  = C^-1/2 q k^T, stored, then softmax_rows_kernel in place,
//   vt [B][C][N]  = v^T,
//   out [B][N][C] = P v (contraction over the N positions: N must be a multiple of the K tile, af_vae_attn_shape_ok).
// Both GEMMs are batched (blockIdx.z) launches of af_launch_conv_gemm without a caller's plan.
struct AfVaeAttnTaps {
  void* scores;      // device [B][N][N] of `dtype` or null: the stored scores before the softmax (copied between the launches)
  void* probs;       // ... P after it
  int plans[2][3];   // (kernel, tile, splitk) of the scores GEMM and of the P v GEMM, from af_get_last_plan()
};
// false + the error message when N positions cannot be contracted over (nothing is launched for such a shape)
bool af_vae_attn_shape_ok(int dtype, int N);
int af_vae_attn_core(int dtype, void* qkv, void* sc, void* vt, void* out, int B, int N, int C, hipStream_t s,
                     AfVaeAttnTaps* taps = nullptr);
template <typename T> int af_launch_to_uint8(const void* x, int ld, uint8_t* y, long npix, hipStream_t s);
int af_launch_nchw_to_uint8(const float* x, uint8_t* y, int B, int HW, hipStream_t s);

// weight repack (device): src fp32 [rows][cin][ks][ks] -> dst T rows [row_off + perm(n)][ks*ks*cin_pad]
//   perm: 0 identity, 1 GEGLU interleave (value/gate groups of 16, half = rows/2)
template <typename T>
int af_launch_repack_weight(const float* src, void* dst, int rows, int cin, int cin_pad, int ks, int ldw, int row_off,
                            int perm, hipStream_t s);
int af_launch_permute_bias(const float* src, float* dst, int rows, int perm, hipStream_t s);
// ... with LoRA adapters merged while it repacks (af_lora.hip): dst = T(src + sum_a scales[a] * up[a] @ down[a]), fp32, rounded
// once; up[a] fp32 [rows][ranks[a]], down[a] fp32 [ranks[a]][cin * ks * ks] on the device, the four arrays on the host (copied
// into the kernel's arguments).  n_adapters 0 .. 8 (0: the bits of af_launch_repack_weight), ranks 1 .. 256.  A refused
// argument: -1 with a message, nothing launched
template <typename T>
int af_launch_lora_repack(const float* src, void* dst, int rows, int cin, int cin_pad, int ks, int ldw, int row_off, int perm,
                          int n_adapters, const float* const* up, const float* const* down, const int* ranks,
                          const float* scales, hipStream_t s);
// LayerNorm folded into a linear: Wf = W * gamma (rounded to T), colsum[n] = sum_k Wf[n][k], biasf = W beta + bias
template <typename T>
int af_launch_ln_fold(const void* W, void* Wf, const float* gamma, const float* beta, const float* bias, float* colsum,
                      float* biasf, int rows, int K, int ldw, hipStream_t s);

// LayerNorm row statistics [parts][M][2] (sum, sum of squares) -> [M][2] (mu, rstd)
int af_launch_ln_finalize(const float* part, int parts, int M, int count, float eps, float* out, hipStream_t s);

// plan of the most recent af_launch_conv_gemm (diagnostics, af_last_gemm_plan)
void af_set_last_plan(const AfGemmPlan& pl);
AfGemmPlan af_get_last_plan();
// launches since af_gemm_plan_counts_reset, read off the plan's kernel by af_launch_conv_gemm
enum AfPlanCount {
  AF_PC_TILE0 = 0,         // [0..5] by AfGemmPlan::tile: four-wave, ping-pong, eight-wave halo, small-map, row-panel and M128 launches
  AF_PC_HALO4 = 6,         // four-wave LDS-halo launches (not counted under their tile)
  AF_PC_SPLITK = 7,        // launches that ran more than one K slice (besides their own slot)
  AF_PC_LN_CONSUMER = 8,   // launches with the LayerNorm consumer epilogue ...
  AF_PC_LN_PRODUCER = 9,   // ... / the statistics-producer epilogue
  AF_PC_FP8 = 10,          // fp8-operand launches (ff_geglu_fp8 included); not counted under a tile
  AF_PC_HALO8 = 11,        // eight-wave halo launches (counted under tile 5 as well)
  AF_PC_ROWPANEL = 12,     // row-panel and M128 launches (counted under their planned tile as well)
  AF_PC_UP_PHASE4 = 13,    // four-phase upsample launches; not counted under a tile
  AF_PC_GN_PRODUCER = 14,  // launches that wrote GroupNorm partial sums
  AF_PC_COUNT = 15
};
extern std::atomic<long> g_af_plan_counts[AF_PC_COUNT];
extern std::atomic<long> g_af_gn_consumer_launches;
int af_launch_up_phase4_weights(const void* w3, int rows, int cin, int ldw3, void* w4, hipStream_t stream);
// fp8 (e4m3) twin of a repacked bf16 weight (K in 64-channel units, power-of-two row scales) / saturating bf16 -> e4m3 cast
int af_launch_quant_weight_fp8(const void* w, int rows, int ldw, int cin_pad, int ks, void* w8, int k8, unsigned char* sc,
                               hipStream_t stream);
int af_launch_cast_fp8(const void* x, void* y, long n, float mul, hipStream_t stream);
