// kernels_mfma.hip — the fused full-batch policy passes (gradient, Fisher-vector product, evaluation) of the 5-128-2
// categorical policy on the bf16 matrix pipe.  The tile machinery is bf16_tile.hpp; the critic step (one output) is
// kernels_critic.hip, which also holds the DQN gradient (two outputs, k_critic_step_mfma<2>); with in-kernel TD targets
// the DQN gradient is k_dqn_step_bf16 in kernels_dqn.hip.
#include <type_traits>

#include "bf16_tile.hpp"
#include "device_fns.hpp"
#include "kernels.hpp"
#include "mask_plane.hpp"
#include "policy_fast.hpp"

constexpr int V2_WAVES = 8;        // policy kernels: one workgroup of eight waves per CU (two per SIMD)

// ================================================================================================
// Policy passes on the bf16 matrix pipe (tile machinery: bf16_tile.hpp; every product exact, f32 accumulation).
//   PASS_INIT / PASS_PPO   gradient of the (clipped) surrogate: forward, per-sample math, masked-sum backward
//   PASS_JVP               Fisher-vector product J^T (diag p - p p^T) J v: tangent forward, per-sample metric, masked-sum
//                          backward — on the relu' masks and the Fisher weights p0 p1 the gradient pass of the same call
//                          KEPT for it (PASS_INIT with KEEP: mask_plane.hpp); the parameters do not move
//                          during the conjugate-gradient solve, so the pass has no forward of its own
//   PASS_EVAL              surrogate loss and KL of candidate parameters: forward only
// Forward output layer (INIT / PPO / EVAL): relu through |x| as in the critic step — for each of the two logits
//   z_a = b2_a + (v_a . x~ + sum_j w2_aj |pre_j|) / 2,  v_ak = sum_j w2_aj W~1[j][k].
// Tangent forward (JVP): the metric only needs the DIFFERENCE of the two tangent logits,
//   dz_0 - dz_1 = sum_j relu'(pre_j) (w2d_j t_j + t2d_j pre_j) + (vb2_0 - vb2_1),   w2d = W2[0] - W2[1], t2d likewise,
// and  w2d_j t_j + t2d_j pre_j = x~ . Z_j  with  Z_jk = w2d_j V~1[j][k] + t2d_j W~1[j][k]  — linear in the inputs, so it
// is a second layer-1 product with Z as the weight matrix (its piece fragments are built once per launch and parked in
// LDS: 12 KB shared by the workgroup's waves), one multiply-clamp and one fma per (sample, unit).
// Backward: the logit gradient of a 2-way softmax is antisymmetric (dz_1 = -dz_0), so one channel g = (dz_0 - dz_1) / 2:
//   M_d[j][k] = sum_s [pre_sj > 0] g_s x~_sk,  dW1[j][k] = (W2[0][j] - W2[1][j]) M_d[j][k],
//   dW2[0][j] = -dW2[1][j] = sum_k W~1[j][k] M_d[j][k];  db2 keeps its two exact per-channel sums.
// Reference semantics: Trpo::update closure + HessianVectorProduct (src/torch/agents/policies/trpo.rs:97-146,
// src/torch/optimizers/conjugate_gradient.rs:262-339), Ppo::update (policies/ppo.rs:124-137), Categorical
// (src/torch/distributions/categorical.rs).
// ================================================================================================
constexpr int PB_FLUSH = 16;  // f32 -> f64 flush period in tiles (32 / 64: 2 % faster Fisher-vector products, measured; TRPO's
                              // CG wants the shorter f32 accumulation)

template <int MODE, int WAVES, bool FW_LDS = false, bool KEEP = false>
__global__ void __launch_bounds__(WAVES * 64)
    k_policy_bf16(TrajDev tr, const float *__restrict__ params, const uint32_t *__restrict__ wimg,
                  const float *__restrict__ tangent, float *__restrict__ lp0, double *__restrict__ slabA,
                  double *__restrict__ slabB, float inv_B, uint32_t P, const int32_t *__restrict__ skip, float clip_lo,
                  float clip_hi, uint32_t share_old, uint32_t share_young, uint32_t *__restrict__ kept_mask,
                  float *__restrict__ kept_w) {
  static_assert(!KEEP || MODE == PASS_INIT, "only the gradient pass keeps");
  using bt::Frag;
  constexpr int D = 5, H = 128, NT = bt::NT, A = 2;
  constexpr bool BWD = MODE != PASS_EVAL;
  constexpr bool JVP = MODE == PASS_JVP;
  constexpr int IW = 7;              // f64 image slots per hidden unit (six columns)
  constexpr int PIMG_M = H * IW + 5; // then db2[0], db2[1], sum0, sum1, sum2
  __shared__ __attribute__((aligned(16))) float Ysh[JVP ? 1 : WAVES][32][bt::YROW];
  __shared__ double Acc[WAVES][BWD ? PIMG_M : 4];
  __shared__ uint4 Fz[JVP ? bt::L2_KS : 1][64];  // JVP: A operands of the masked sum over the hidden units (pieces of Z)
  __shared__ uint4 Fw[FW_LDS ? NT * 3 : 1][64];  // FW_LDS: the weight fragments live in LDS, shared by the waves
  if (skip != nullptr && *skip != 0) return;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform: tile indices stay scalar
  const int n = lane & 31, hf = lane >> 5;
  const float *__restrict__ W1 = params, *__restrict__ b1 = W1 + bt::PAR_B1, *__restrict__ W2 = params + bt::PAR_W2,
                           *__restrict__ b2 = params + bt::par_b2(A);
  const size_t B = (size_t)tr.T * tr.n;
  const size_t plane = (size_t)(tr.T + 1) * tr.n;
  double *acc64 = Acc[wave];
  bool flushed = false;  // (the wave's f64 image is not zeroed: its first flush stores, bt::flush)

  Frag fw[NT][3];
  // Only the DIFFERENCE of the two logits enters a two-way log-softmax (it is shift-invariant), so the output layer is
  // one chain with the differenced weights w2d = W2[0] - W2[1]; the passes agree with each other because all of them
  // (and log pi_0, stored by PASS_INIT) use this form.  The rollout's bit-exact forward is device_fns.hpp, not this.
  float w2d[NT];
  float lvd[3] = {0.0f, 0.0f, 0.0f};  // the linear half of relu (bf16_tile.hpp) for the differenced logit
  float tb2d = 0.0f;
  // (the Fisher-vector pass reads no weights: its masks are the kept ones, and the range guard has run in the gradient
  // pass of the same call)
  auto fold_raw = [&](int t, const bt::WRaw &r) {
    if (FW_LDS && wave == t) {
#pragma unroll
      for (int i = 0; i < 3; ++i) Fw[t * 3 + i][lane] = fw[t][i].x;
    }
    // the forward runs on weights scaled by 2^96 (relu' by conversion, bf16_tile.hpp); the |pre| chain of the gradient /
    // evaluation passes takes the scale back out through w2d (both exact)
    const float wd = r.w2[0] - r.w2[1];
    lvd[0] = __builtin_fmaf(wd, r.wa, lvd[0]);
    lvd[1] = __builtin_fmaf(wd, r.wb, lvd[1]);
    lvd[2] = __builtin_fmaf(wd, r.wc, lvd[2]);
    w2d[t] = bt::FWD_UNSCALE * wd;
  };
  if (!JVP) bt::load_weights<bt::GUARD_POLICY>(wimg, wave, lane, 2, tr.range, tr.range_err, fw, fold_raw);
  if (JVP) {
    // Z_jk = w2d_j V~1[j][k] + t2d_j W~1[j][k] (k = 5: the bias row): the tangent logit difference is
    // sum_j relu'(pre_j) (x~ . Z_j) + (vb2_0 - vb2_1) = sum_k x~_k q_k + ..., q = the masked sum of Z's rows
    const float *__restrict__ V1 = tangent, *__restrict__ vb1 = V1 + bt::PAR_B1, *__restrict__ V2 = tangent + bt::PAR_W2;
    bt::l2_build(Fz, (int)threadIdx.x, WAVES * 64, [&](int j, int k) {
      const float wd = W2[j] - W2[H + j], t2d = V2[j] - V2[H + j];
      const float w = k < D ? W1[j * D + k] : b1[j], v = k < D ? V1[j * D + k] : vb1[j];
      return __builtin_fmaf(t2d, w, wd * v);
    });
  }
  if (JVP || FW_LDS) __syncthreads();
  if (JVP) {
    const float *__restrict__ vb2 = tangent + bt::par_b2(A);
    tb2d = vb2[0] - vb2[1];
  } else {
#pragma unroll
    for (int q = 0; q < 3; ++q) lvd[q] = bt::half_sum(lvd[q]);
  }
  const float b2d = b2[0] - b2[1];
  Frag selb[2], idb[2];  // piece-column selection, identity (B operands of the routing / transposing products)
  if (BWD) bt::sel_frags(lane, selb);
  if (JVP) bt::ident_frags(lane, idb);
  bt::f32x16 dm[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) dm[t] = (bt::f32x16){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  double sum0 = 0.0, sum1 = 0.0, sum2 = 0.0, db2_0 = 0.0, db2_1 = 0.0;  // owner-lane f64 sums ...
  // ... fed through per-lane f32 partials over one flush period (PB_FLUSH tiles): the two levels of every sum over
  // samples in this library, and a conversion + an f64 addition less per sum and tile
  float s0f = 0.0f, s1f = 0.0f, s2f = 0.0f, d0f = 0.0f, d1f = 0.0f;
  auto fold = [&]() {
    sum0 += (double)s0f;
    sum1 += (double)s1f;
    sum2 += (double)s2f;
    db2_0 += (double)d0f;
    db2_1 += (double)d1f;
    s0f = s1f = s2f = d0f = d1f = 0.0f;
  };
  bt::wave_lds_fence();

  // Tiles (bt::walk_tiles): indices are wave-uniform (SGPRs); the operands come through buffer loads with a constant
  // per-lane byte offset and the tile's offset as the scalar operand: no vector address arithmetic per tile.
  const uint32_t B32 = (uint32_t)B, plane32 = (uint32_t)plane;
  const uint32_t n_full = B32 / 32u, tail = B32 & 31u;
  // (the tiles are dealt 5 : 3 between the older and the younger wave of a SIMD: bf16_tile.hpp SHARE_OLD; the
  // sixteen-wave evaluation pass deals evenly — its launcher passes 1 : 1)
  if (WAVES != 8) share_old = share_young = 1u;  // (compile-time for the sixteen-wave form: the walk's outer loop folds away)
  const bt::Dealing deal = bt::deal_tiles<WAVES>(wave, share_old, share_young);
  const bt::rsrc_t obs_r = bt::make_rsrc(tr.obs, (uint32_t)D * plane32 * 4u), lp0_r = bt::make_rsrc(lp0, 2u * B32 * 4u);
  const bt::rsrc_t adv_r = bt::make_rsrc(tr.adv, B32 * 4u), act_r = bt::make_rsrc(tr.action, B32);
  const uint32_t off_a = ((uint32_t)(2 * hf) * plane32 + (uint32_t)n) * 4u, off_b = off_a + plane32 * 4u;
  const uint32_t off_c = (4u * plane32 + (uint32_t)n) * 4u, off_s = (uint32_t)n * 4u, off_s1 = off_s + B32 * 4u;
  // the kept planes (KEEP writes, the Fisher-vector pass reads): 8 bytes of mask bits per (tile, lane), one Fisher weight
  // per sample
  const uint32_t n_tiles32 = (B32 + 31u) / 32u;
  const bt::rsrc_t km_r = bt::make_rsrc(kept_mask, n_tiles32 * mp::TILE_BYTES), kw_r = bt::make_rsrc(kept_w, B32 * 4u);
  const uint32_t off_m = mp::lane_offset(lane);
  int since_flush = 0;
  // per lane: features 2 hf, 2 hf + 1 and 4 of sample n, and the per-sample scalars the pass needs (log pi_0 of both
  // actions; advantage and action; the Fisher-vector pass: the lane's kept mask words and its sample's kept weight) — all
  // requested one tile ahead
  struct TileOp {
    float xa, xb, xc, l0, l1, adv;
    int act;
    uint32_t m[mp::WORDS];
    float w;
  };
  auto load_tile = [&](uint32_t g) {  // g: wave-uniform tile index
    TileOp o;
    const uint32_t soff = g * 128u;
    o.xa = bt::buf_f32(obs_r, off_a, soff);
    o.xb = bt::buf_f32(obs_r, off_b, soff);
    o.xc = bt::buf_f32(obs_r, off_c, soff);
    o.l0 = o.l1 = o.adv = o.w = 0.0f;
    o.act = 0;
    o.m[0] = o.m[1] = 0u;
    if (JVP) {
      const bt::u32x2 mw = bt::buf_u32x2(km_r, off_m, mp::tile_offset(g));
      o.m[0] = mw[0];
      o.m[1] = mw[1];
      o.w = bt::buf_f32(kw_r, off_s, soff);
    } else if (MODE != PASS_INIT) {  // log pi_0 (written by PASS_INIT, read by the others)
      o.l0 = bt::buf_f32(lp0_r, off_s, soff);
      o.l1 = bt::buf_f32(lp0_r, off_s1, soff);
    }
    if (!JVP) {
      o.adv = bt::buf_f32(adv_r, off_s, soff);
      o.act = (int)bt::buf_u8(act_r, (uint32_t)n, g * 32u);
    }
    return o;
  };
  auto tile = [&](auto ragged, TileOp op_in, uint32_t g) {
    constexpr bool RAGGED = decltype(ragged)::value;
    struct {
      float xa, xb, xc, l0, l1, adv;
      int act;
      bool valid;
    } op;
    op.valid = RAGGED ? (uint32_t)n < tail : true;
    // (the arrays extend past sample B - 1 or the loads return 0 there: a padding lane's operands are zeroed)
    op.xa = op.valid ? op_in.xa : 0.0f;
    op.xb = op.valid ? op_in.xb : 0.0f;
    op.xc = op.valid ? op_in.xc : 0.0f;
    op.l0 = op.valid ? op_in.l0 : 0.0f;
    op.l1 = op.valid ? op_in.l1 : 0.0f;
    op.adv = op.valid ? op_in.adv : 0.0f;
    op.act = op.valid ? op_in.act : 0;
    const float kw_in = op.valid ? op_in.w : 0.0f;
    const size_t sidx = (size_t)g * 32 + n;
    Frag fa[3];
    if (!JVP) bt::input_frags(op.xa, op.xb, op.xc, op.valid, hf, fa);
    Frag ga[NT][2];
    float y0[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) y0[r] = 0.0f;
    bt::f32x16 q = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    auto fwd = [&](int t) {
      if (FW_LDS) {
        Frag f[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) f[i].x = Fw[t * 3 + i][lane];
        return bt::layer1(fa, f);
      }
      return bt::layer1(fa, fw[t]);
    };
    if (JVP) {
      // the kept masks (a padding sample's bits are 0: the keeping pass saw pre = 0 there), decoded into the register
      // contents bt::mask_tile would leave: two vector instructions per pair, one shift per eight
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int i = 0; i < 4; ++i) ga[t][s].u[i] = mp::decode_pair(op_in.m, mp::pair_index(t, s, i));
        q = bt::masked_sum_tile(ga[t], idb, Fz, t, lane, q);
      }
    } else {
      uint32_t grp[NT];  // KEEP: the tile's mask bits, a group word per hidden tile (mask_plane.hpp)
      bt::f32x16 c = fwd(0);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        bt::f32x16 cn = c;
        if (t + 1 < NT) cn = fwd(t + 1);
#pragma unroll
        for (int r = 0; r < 16; ++r) y0[r] = __builtin_fmaf(__builtin_fabsf(c[r]), w2d[t], y0[r]);
        if (BWD) bt::mask_tile(c, ga[t]);  // relu'(pre): one conversion per two values
        if (KEEP) grp[t] = mp::encode_group([&](int k) { return ga[t][k >> 2].u[k & 3]; });
        c = cn;
      }
      if (KEEP) {
        const bt::u32x2 mw = {mp::encode_word(grp[0], grp[1]), mp::encode_word(grp[2], grp[3])};
        bt::buf_store_u32x2(mw, km_r, off_m, mp::tile_offset(g));
      }
    }
    float s0;
    if (JVP) {
      float p0, p1;
      bt::both_halves(bt::l2_dot(q, op.xa, op.xb, hf == 0 ? op.xc : 1.0f), p0, p1);
      s0 = p0 + p1;
    } else {
      s0 = 0.5f * bt::transpose_sum(
                      Ysh, JVP ? 0 : wave, y0, [&] { return bt::linear_half(lvd, op.xa, op.xb, op.xc, hf); }, n, hf);
      bt::wave_lds_fence();  // Ysh is rewritten by the next tile
    }
    // ---- per-sample math on the owner lanes (lane n and n + 32 both hold sample n)
    float dz0 = 0.0f, dz1 = 0.0f;
    if (JVP) {
      const float delta = s0 + tb2d;
      dz0 = op.valid ? kw_in * delta * inv_B : 0.0f;  // kw_in = p0 p1 of pi_0, kept by the gradient pass
      dz1 = -dz0;
    } else {
      const float adv = op.adv;
      const int act = op.act;
      const SoftPair sp = soft_pair(s0 + b2d);
      const float(&lp)[2] = sp.lp;
      if (MODE == PASS_PPO) {
        // clipped surrogate (policies/ppo.rs:124-137); see k_policy_pass for the tie rules of minimum()/clamp()
        const float l0a = act == 0 ? op.l0 : op.l1;
        const float lpa = act == 0 ? lp[0] : lp[1];
        const float ratio = fast_expf(lpa - l0a);
        const float clipped = ratio < clip_lo ? clip_lo : (ratio > clip_hi ? clip_hi : ratio);
        const float u1 = ratio * adv, u2 = clipped * adv;
        const bool inside = ratio >= clip_lo && ratio <= clip_hi;
        const float gr = u1 < u2 ? adv : (u1 > u2 ? (inside ? adv : 0.0f) : (inside ? adv : 0.5f * adv));
        const float cc = -(gr * ratio) * inv_B;
        dz0 = op.valid ? cc * ((act == 0 ? 1.0f : 0.0f) - sp.p[0]) : 0.0f;
        dz1 = op.valid ? cc * ((act == 1 ? 1.0f : 0.0f) - sp.p[1]) : 0.0f;
        if (op.valid) s0f = s0f + (u1 < u2 ? u1 : u2);  // (both halves count sample n; the final reduction reads half 0)
      } else if (MODE == PASS_INIT) {
        if (op.valid && hf == 0) {
          lp0[sidx] = lp[0];
          lp0[B + sidx] = lp[1];
          if (KEEP) {  // the Fisher weight of the sample, from the values just stored
            const SoftPair old = soft_pair(lp[0] - lp[1]);  // pi_0 from its stored log-probabilities
            kept_w[sidx] = old.p[0] * old.p[1];
          }
        }
        const float lpa = act == 0 ? lp[0] : lp[1];
        const float ratio = fast_expf(lpa - lpa);
        const float cc = -(ratio * adv) * inv_B;
        const float pa0 = sp.p[0], pa1 = sp.p[1];
        dz0 = op.valid ? cc * ((act == 0 ? 1.0f : 0.0f) - pa0) : 0.0f;
        dz1 = op.valid ? cc * ((act == 1 ? 1.0f : 0.0f) - pa1) : 0.0f;
        const float cl0 = lp[0] < -3.402823466e+38f ? -3.402823466e+38f : lp[0];
        const float cl1 = lp[1] < -3.402823466e+38f ? -3.402823466e+38f : lp[1];
        float ent = cl0 * pa0;
        ent += cl1 * pa1;
        if (op.valid) {
          s0f = __builtin_fmaf(ratio, adv, s0f);
          s1f = s1f - ent;
          s2f = __builtin_fmaf(lpa, adv, s2f);
        }
      } else {  // PASS_EVAL
        const float l00 = op.l0, l01 = op.l1;
        const float lpa = act == 0 ? lp[0] : lp[1];
        const float l0a = act == 0 ? l00 : l01;
        const float ratio = fast_expf(lpa - l0a);
        float rel0 = l00 - lp[0], rel1 = l01 - lp[1];
        if (rel0 < -3.402823466e+38f) rel0 = -3.402823466e+38f;
        if (rel1 < -3.402823466e+38f) rel1 = -3.402823466e+38f;
        const SoftPair old = soft_pair(l00 - l01);  // pi_0 from its stored log-probabilities
        float kl = rel0 * old.p[0];
        kl += rel1 * old.p[1];
        if (op.valid) {
          s0f = __builtin_fmaf(ratio, adv, s0f);
          s1f = s1f + kl;
        }
      }
    }
    if (BWD) {
      d0f = d0f + dz0;  // (dz is 0 on padding lanes)
      d1f = d1f + dz1;
      // one channel: u[sample][k] = g * x~_k with g = (dz_0 - dz_1) / 2, masked sum over the samples on the matrix pipe
      Frag ub[2];
      bt::piece_frags_mfma(0.5f * (dz0 - dz1), op.xa, op.xb, op.xc, hf, selb, ub);
      bt::backward(ga, ub, dm);
      if (++since_flush == PB_FLUSH) {
        since_flush = 0;
        bt::flush(dm, acc64, IW, n, hf, !flushed);
        flushed = true;
        fold();
      }
    } else if (++since_flush == PB_FLUSH) {
      since_flush = 0;
      fold();
    }
  };
  // (two operand buffers in every pass: without its forward weight fragments the Fisher-vector pass has the registers for
  // the second one — 189 -> 178 us per launch at 8.4 M samples)
  bt::walk_tiles(deal, n_full, tail, load_tile, tile);
  if (BWD && (since_flush != 0 || !flushed)) bt::flush(dm, acc64, IW, n, hf, !flushed);  // (nothing left when the last
                                                                // tile ended a flush period; a wave without tiles
                                                                // still defines its image)
  fold();
  const double r0 = bt::owner_sum(sum0, hf), r1 = bt::owner_sum(sum1, hf);
  const double r2 = bt::owner_sum(db2_0, hf), r3 = bt::owner_sum(db2_1, hf);
  const double r4 = MODE == PASS_INIT ? bt::owner_sum(sum2, hf) : 0.0;
  constexpr int TAIL = BWD ? H * IW : 0;
  if (lane == 0) {
    if (BWD) {
      acc64[TAIL + 0] = r2;
      acc64[TAIL + 1] = r3;
      acc64[TAIL + 2] = r0;
      acc64[TAIL + 3] = r1;
      if (MODE == PASS_INIT) acc64[TAIL + 4] = r4;
    } else {
      acc64[0] = r0;
      acc64[1] = r1;
    }
  }
  __syncthreads();
  auto tot = [&](int src) { return bt::image_sum<WAVES>(Acc, src); };
  if (BWD) {
    for (uint32_t p = threadIdx.x; p < P; p += WAVES * 64) {
      double s;
      if (p < bt::par_b2(A)) {  // M_0 = M_d, M_1 = -M_d
        s = bt::grad_entry<1>(p, params, [&](int, int j, int k) { return tot(j * IW + k); },
                              [&](int, int j) { return (double)W2[j] - (double)W2[H + j]; });
        if (p >= bt::PAR_W2 + H) s = -s;
      } else {
        s = tot(TAIL + (int)(p - bt::par_b2(A)));
      }
      slabA[(size_t)blockIdx.x * P + p] = s;
    }
  }
  if (threadIdx.x < 4) {
    double v = 0.0;
    if (BWD) {
      if (!JVP && threadIdx.x < 2) v = tot(TAIL + 2 + threadIdx.x);
      if (MODE == PASS_INIT && threadIdx.x == 2) v = tot(TAIL + 4);
    } else if (threadIdx.x < 2) {
      v = tot(threadIdx.x);
    }
    slabB[(size_t)blockIdx.x * 4 + threadIdx.x] = v;
  }
}

// The kept planes of a trajectory (mask_plane.hpp; engine.hpp says who may trust them): room for the samples the
// trajectory was allocated for, on first use
static void traj_ensure_kept_planes(rl_traj *t) {
  const uint64_t samples = (uint64_t)t->d.n * t->d.T;
  t->mem.ensure(t->kept_mask, mp::plane_words(samples));
  t->mem.ensure(t->kept_w, samples);
}

// gradient (PASS_INIT), Fisher-vector product (PASS_JVP) or loss/KL evaluation (PASS_EVAL) in one launch
bool launch_policy_v2(rl_traj *traj, const rl_mlp *policy, int mode, const float *d_tangent, uint64_t B_total,
                      const int32_t *d_skip, float clip_lo, float clip_hi, bool keep) {
  if (policy->general) return launch_gen_mfma(traj, policy, mode, d_tangent, B_total, d_skip, clip_lo, clip_hi);
  if (!fused_5_128_fits(traj, policy, 2)) return false;  // (only feed-forward modules are passed here)
  if (mode == PASS_DQN) return false;  // k_dqn_step_bf16 (kernels_dqn.hip)
  keep = keep && mode == PASS_INIT;
  if (keep) {
    traj->kept_epoch = 0;  // (until the launch is enqueued: a failure on the way leaves nothing to trust)
    traj_ensure_kept_planes(traj);
  }
  if (mode == PASS_JVP && !(traj->kept_epoch == traj->eng->call_epoch && traj->kept_policy == policy &&
                            traj->kept_samples == traj->B && traj->kept_mask != nullptr && traj->kept_w != nullptr))
    throw RlError(RL_ERR_UNSUPPORTED,
                  "internal error: a Fisher-vector pass without a keeping gradient pass of the same policy and trajectory "
                  "before it in the same call (its relu' masks would be stale)");
  traj_ensure_range(traj);
  const uint32_t *wimg = wimg_ensure(policy);
  ProfScope ps(traj->eng, mode == PASS_JVP ? RL_K_POLICY_FVP : RL_K_POLICY_FUSED);
  float inv_B = 1.0f / (float)B_total;
  traj->nbV2 = fused_grid(traj, V2_WAVES);  // (what traj_plan planned: one tile per wave and iteration)
  traj->last_rows = traj->nbV2;
  dim3 g(traj->nbV2), b(V2_WAVES * 64);
  hipStream_t s = traj->eng->stream;
  uint32_t P = (uint32_t)policy->P;
  const TrajDev d = fused_traj_dev(traj, traj->guard_next_policy);
#define BLAUNCH(MM)                                                                                                  \
  hipLaunchKernelGGL((k_policy_bf16<MM, V2_WAVES>), g, b, 0, s, d, policy->d_params, wimg, d_tangent, traj->lp0,       \
                     traj->slabA, traj->slabB, inv_B, P, d_skip, clip_lo, clip_hi, bt::SHARE_OLD, bt::SHARE_YOUNG,      \
                     traj->kept_mask, traj->kept_w)
  if (keep) {
    hipLaunchKernelGGL((k_policy_bf16<PASS_INIT, V2_WAVES, false, true>), g, b, 0, s, d, policy->d_params, wimg,
                       d_tangent, traj->lp0, traj->slabA, traj->slabB, inv_B, P, d_skip, clip_lo, clip_hi, bt::SHARE_OLD,
                       bt::SHARE_YOUNG, traj->kept_mask, traj->kept_w);
    traj->kept_epoch = traj->eng->call_epoch;
    traj->kept_policy = policy;
    traj->kept_samples = traj->B;
  } else if (mode == PASS_INIT) {
    traj->kept_epoch = 0;  // (log pi_0 is rewritten without the planes that go with it)
    BLAUNCH(PASS_INIT);
  } else if (mode == PASS_JVP) BLAUNCH(PASS_JVP);
  else if (mode == PASS_PPO) BLAUNCH(PASS_PPO);
  else {
    // the evaluation pass has no backward state: with the weight fragments in LDS it fits twelve waves per CU (152
    // VGPRs) — 0.155 ms per launch at 8.4 M samples against 0.206 ms at eight (sixteen waves: 17 spills, no gain)
    constexpr int EVAL_WAVES = 16;
    hipLaunchKernelGGL((k_policy_bf16<PASS_EVAL, EVAL_WAVES, true>), g, dim3(EVAL_WAVES * 64), 0, s, d,
                       policy->d_params, wimg, d_tangent, traj->lp0, traj->slabA, traj->slabB, inv_B, P, d_skip, clip_lo,
                       clip_hi, 1u, 1u, nullptr, nullptr);
  }
#undef BLAUNCH
  return true;
}
