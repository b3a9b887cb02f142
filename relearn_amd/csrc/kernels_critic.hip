// kernels_critic.hip — the fused critic step: forward + MSE loss + backward of the 5-128-1 value MLP over all samples.
//
// Reference semantics: ValuesOpt::update (src/torch/agents/critics/opt.rs:100-126): loss = mse_loss(V(obs), targets,
// Mean); backward; the optimiser step itself is k_reduce_opt / k_opt_step (kernels_update.hip).
//
// Tile machinery (layer 1 and the masked-sum backward on the bf16 matrix pipe with exact three-piece splits — no
// reduced precision): bf16_tile.hpp.  On top of it, per 32-sample tile and wave:
//   relu through |x|:  relu(x) = (x + |x|) / 2, so  y = b2 + (sum_j w2_j pre_j + sum_j w2_j |pre_j|) / 2 — the first sum
//   is linear in the inputs (v . x~ with v_k = sum_j w2_j W~1[j][k], six numbers per launch), the second costs one fma
//   with an |.| source per (sample, unit): no separate relu; the partial sums of a lane's four units go through one
//   per-wave LDS transpose; per-sample loss and dL/dy on the sample-owning lanes; the backward's mask is HALF an
//   instruction per (sample, unit): the forward is scaled by 2^96 and v_cvt_pk_bf16_f32 with the clamp bit packs two
//   relu' values at once (bf16_tile.hpp).
//   at the end  dL/dW1[j][k] = w2_j M[j][k],  dL/db1[j] = w2_j M[j][5],  dL/db2 = sum dy,
//               dL/dW2[j] = sum_s dy_s h_sj = sum_k W~1[j][k] M[j][k]   (h_sj = [pre_sj > 0] W~1[j] . x~_s).
// (The output layer as a masked sum on the matrix pipe — what the Fisher-vector pass gains 17 % from, kernels_mfma.hip —
// loses here: 0.259 against 0.219 ms per step; this kernel has one |pre| chain to replace, not a second layer-1 product
// with its LDS-resident operands, and 16 more matrix instructions per tile push it against the matrix pipe.)
// Algorithmic flops per sample: 3 x (2*5*128 + 2*128) = 4608 (forward + 2 x backward of the 5-128-1 MLP).
#include <type_traits>

#include "bf16_tile.hpp"
#include "device_fns.hpp"
#include "kernels.hpp"

static_assert(bt::RANGE_WORDS == RL_RANGE_WORDS && bt::RANGE_ALLOC_WORDS == RL_RANGE_ALLOC_WORDS &&
                  bt::GUARD_POLICY == RL_GUARD_POLICY && bt::GUARD_CRITIC == RL_GUARD_CRITIC,
              "engine.hpp and bf16_tile.hpp describe the same range / veto words");

using bt::f32x16;
using bt::Frag;

constexpr int CRITIC_WAVES = 8;  // waves per workgroup, one workgroup per CU (two waves per SIMD: the
                                               // tile state — 64 accumulators of each pass, 48 weight-piece registers —
                                               // does not fit three)
constexpr int C_FLUSH = 64;  // f32 -> f64 flush period in tiles (2048 samples per accumulator: the accumulated error stays below a 128-sample f32 fma chain's, scripts/probe/mfma_bf16_mask.hip)

// CH = 1: the critic step (above).  CH = 2 (round 6): the DQN gradient — mean((Q(s)[a] - target)^2) of the 5-128-2
// action-value MLP, dqn.rs:316-326 — as TWO critic steps side by side: the loss reaches the hidden layer through row a_s
// of the output weights only, so channel c (waves 0-3: c = 0, waves 4-7: c = 1) is the critic step of the one-output
// network (W1, b1, W2[c], b2[c]) over the samples with a_s = c, every other sample contributing zero.  Both channels walk
// the same tiles (the forward is computed twice) — and the two waves of a SIMD, one of each channel, overlap each other's
// matrix and vector work, which the one-wave-per-SIMD kernel of rounds 3-5 (two backward channels in one wave's whole
// register file: k_dqn_step_bf16, still the kernel of the in-kernel TD targets) could not: 19.0 -> 11 us per launch.
// The workgroup's row combines them: dW1[j][k] = W2[0][j] M_0[j][k] + W2[1][j] M_1[j][k] (db1 likewise),
// dW2[c][j] = sum_k W~1[j][k] M_c[j][k], db2[c] = sum of channel c's dL/dy, the loss the sum of both channels'.
template <int CH>
__global__ void __launch_bounds__(CRITIC_WAVES * 64, 2)
    k_critic_step_mfma(TrajDev tr, const float *__restrict__ params, const uint32_t *__restrict__ wimg,
                       double *__restrict__ slabA, double *__restrict__ slabB, float two_over_B, uint32_t P,
                       uint32_t share_old, uint32_t share_young) {
  constexpr int D = 5, H = 128, NT = bt::NT;
  constexpr int IMG = H * 7 + 2;  // per hidden unit: M[0..5] (slot 6 unused); then db2, loss
  __shared__ __attribute__((aligned(16))) float Ysh[CRITIC_WAVES][32][bt::YROW];
  __shared__ double Acc[CRITIC_WAVES][IMG];  // f64 level of the two-level accumulation, one image per wave

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform: tile indices stay scalar
  const int n = lane & 31, hf = lane >> 5;
  const float *__restrict__ W2 = params + bt::PAR_W2;
  const int chan = CH == 2 ? (wave >= CRITIC_WAVES / 2 ? 1 : 0) : 0;  // (wave-uniform) the output this wave differentiates
  const float b2 = W2[CH * H + chan];
  const size_t B = (size_t)tr.T * tr.n;
  const size_t plane = (size_t)(tr.T + 1) * tr.n;
  double *acc64 = Acc[wave];
  // (the wave's f64 image is not zeroed: its first flush stores — bt::flush — and every wave flushes at least once)
  bool flushed = false;

  // weight pieces of hidden unit 32 t + n in this half's slot order; w2; the linear half of relu (v of this half's
  // inputs: 2 hf, 2 hf + 1, and 4 or the bias)
  Frag fw[NT][3];
  float w2v[NT];
  float lv[3] = {0.0f, 0.0f, 0.0f};
  // (the range guard: the two-channel form is the DQN gradient — the policy chain's words)
  bt::load_weights<CH == 2 ? bt::GUARD_POLICY : bt::GUARD_CRITIC>(
      wimg, wave, lane, CH, tr.range, tr.range_err, fw, [&](int t, const bt::WRaw &r) {
        const float w2 = CH == 2 && chan == 1 ? r.w2[1] : r.w2[0];
        lv[0] = __builtin_fmaf(w2, r.wa, lv[0]);
        lv[1] = __builtin_fmaf(w2, r.wb, lv[1]);
        lv[2] = __builtin_fmaf(w2, r.wc, lv[2]);
        // the forward runs on weights scaled by 2^96 (relu' by conversion, bf16_tile.hpp); the |pre| chain takes the
        // scale back out through w2 (both exact)
        w2v[t] = bt::FWD_UNSCALE * w2;
      });
#pragma unroll
  for (int q = 0; q < 3; ++q) lv[q] = bt::half_sum(lv[q]);
  // backward accumulators (matrix pipe): dm[t][r] = sum over samples for hidden unit 32 t + row(r, hf), piece column n
  f32x16 dm[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) dm[t] = (f32x16){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  double loss64 = 0.0, db2_64 = 0.0;
  float loss32 = 0.0f, db2_32 = 0.0f;  // per-lane f32 partials over one flush period (<= 64 tiles), then f64: the two levels
                                         // of every sum over samples here
  bt::wave_lds_fence();

  Frag selb[2];  // piece-column selection (B operand of the routing product)
  bt::sel_frags(lane, selb);
  // Tiles (bt::walk_tiles): indices are wave-uniform (SGPRs); the operands come through buffer loads with a constant
  // per-lane byte offset and the tile's offset as the scalar operand: no vector address arithmetic per tile.
  const uint32_t B32 = (uint32_t)B, plane32 = (uint32_t)plane;
  const uint32_t n_full = B32 / 32u, tail = B32 & 31u;
  // The two waves of a SIMD do not progress alike: the older one (waves 0-3 of the workgroup, launched first) wins the
  // issue arbitration and used to finish its tiles at 0.71 of the launch, leaving the younger one alone — one wave per
  // SIMD, nothing to overlap its matrix instructions with — for the rest (profiles/r06_critic_step_timeline.txt).  So the
  // tiles are not dealt evenly: an older wave plays `share_old` virtual waves, a younger one `share_young`, and both
  // finish together (bt::deal_tiles).  (CH = 2: the two channels walk the same tiles, dealt evenly.)
  if (CH == 2) share_old = share_young = 1u;
  const bt::Dealing deal = bt::deal_tiles<CRITIC_WAVES, CH>(wave, share_old, share_young);
  const bt::rsrc_t obs_r = bt::make_rsrc(tr.obs, (uint32_t)D * plane32 * 4u), tgt_r = bt::make_rsrc(tr.tgt, B32 * 4u);
  const bt::rsrc_t act_r = bt::make_rsrc(tr.action, B32);  // (CH = 2 only: the action taken selects the channel)
  const uint32_t off_a = ((uint32_t)(2 * hf) * plane32 + (uint32_t)n) * 4u, off_b = off_a + plane32 * 4u;
  const uint32_t off_c = (4u * plane32 + (uint32_t)n) * 4u, off_t = (uint32_t)n * 4u;
  int since_flush = 0;
  // per lane: features 2 hf, 2 hf + 1 and 4 of sample n, and its target
  struct TileOp {
    float xa, xb, xc, tgt;
    uint32_t act;
  };
  auto load_tile = [&](uint32_t g) {  // g: wave-uniform tile index (< 2^25: the launcher bounds the element count)
    TileOp o;
    const uint32_t soff = g * 128u;
    o.xa = bt::buf_f32(obs_r, off_a, soff);
    o.xb = bt::buf_f32(obs_r, off_b, soff);
    o.xc = bt::buf_f32(obs_r, off_c, soff);
    o.tgt = bt::buf_f32(tgt_r, off_t, soff);
    o.act = CH == 2 ? bt::buf_u8(act_r, (uint32_t)n, g * 32u) : 0u;
    return o;
  };

  auto tile = [&](auto ragged, TileOp op, uint32_t) {
    constexpr bool RAGGED = decltype(ragged)::value;
    const bool valid = RAGGED ? (uint32_t)n < tail : true;
    if (RAGGED) {  // (the observation planes extend past sample B - 1: what a padding lane read is not zero)
      op.xa = valid ? op.xa : 0.0f;
      op.xb = valid ? op.xb : 0.0f;
      op.xc = valid ? op.xc : 0.0f;
      op.tgt = valid ? op.tgt : 0.0f;
    }
    Frag fa[3];
    bt::input_frags(op.xa, op.xb, op.xc, valid, hf, fa);
    // ---- forward, one hidden tile at a time, software-pipelined: the matrix pipe works on hidden tile t + 1 while the
    // VALU does the partial y and the relu' mask of hidden tile t; the mask is packed as the backward's A operand
    Frag ga[NT][2];
    float yp[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) yp[r] = 0.0f;
    f32x16 c = bt::layer1(fa, fw[0]);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x16 cn = c;
      if (t + 1 < NT) cn = bt::layer1(fa, fw[t + 1]);
#pragma unroll
      for (int r = 0; r < 16; ++r) yp[r] = __builtin_fmaf(__builtin_fabsf(c[r]), w2v[t], yp[r]);
      bt::mask_tile(c, ga[t]);  // relu'(pre): one conversion per two values
      c = cn;
    }
    // ---- y: the 16 partial sums per lane go through an LDS transpose (folding them in registers instead was measured in
    // round 5 — the same time per step — and removed: DESIGN 17)
    const float y =
        0.5f * bt::transpose_sum(Ysh, wave, yp, [&] { return bt::linear_half(lv, op.xa, op.xb, op.xc, hf); }, n, hf) + b2;
    const float d = y - op.tgt;
    // (CH = 2: only the samples whose action is this wave's channel count — loss, db2 and the backward alike)
    const bool mine = CH == 2 ? valid && op.act == (uint32_t)chan : valid;
    const float dy = mine ? d * two_over_B : 0.0f;
    if (mine) {  // (both halves hold sample n and count it; the reduction after the loop reads half 0 only)
      loss32 = __builtin_fmaf(d, d, loss32);
      db2_32 = db2_32 + dy;
    }
    // ---- backward: u[sample][k] = dy * x~_k as exact pieces (routed to the piece columns by a selection product),
    // masked sum over the samples on the matrix pipe
    Frag ub[2];
    bt::piece_frags_mfma(dy, op.xa, op.xb, op.xc, hf, selb, ub);
    bt::backward(ga, ub, dm);
    bt::wave_lds_fence();  // Ysh is rewritten by the next tile
    if (++since_flush == C_FLUSH) {
      since_flush = 0;
      bt::flush(dm, acc64, 7, n, hf, !flushed);
      flushed = true;
      loss64 += (double)loss32;
      db2_64 += (double)db2_32;
      loss32 = db2_32 = 0.0f;
    }
  };

  // (loading two tiles ahead — by register moves or by rotating three named buffers through a loop unrolled three
  // times — is SLOWER than the walk's one, 0.237 against 0.220 ms per step, although a timing build without the loads
  // runs in 0.197: what the loads cost is issue slots, not exposed latency)
  bt::walk_tiles(deal, n_full, tail, load_tile, tile);
  if (since_flush != 0 || !flushed) {  // (a wave whose tile count is a multiple of the flush period has nothing left: at
                                       // the headline size every wave owns exactly 2 x C_FLUSH tiles, and this was a
                                       // third flush of zeros; a wave without tiles still defines its image)
    bt::flush(dm, acc64, 7, n, hf, !flushed);
    loss64 += (double)loss32;
    db2_64 += (double)db2_32;
  }
  const double l = bt::owner_sum(loss64, hf), bsum = bt::owner_sum(db2_64, hf);
  if (lane == 0) {
    acc64[H * 7] = bsum;   // db2
    acc64[H * 7 + 1] = l;  // loss partial
  }
  __syncthreads();
  // sum the per-wave images in wave order, turn M into gradients and write the workgroup's slab row
  for (uint32_t p = threadIdx.x; p <= P; p += CRITIC_WAVES * 64) {
    auto tot = [&](int src) { return bt::image_sum<CRITIC_WAVES>(Acc, src); };
    auto totc = [&](int c, int src) { return bt::image_sum<CRITIC_WAVES / 2>(Acc + 4 * c, src); };  // channel c's waves
    double s;
    if (p >= bt::par_b2(CH)) {
      s = p == P ? tot(H * 7 + 1) : CH == 2 ? totc((int)(p - bt::par_b2(CH)), H * 7) : tot(H * 7);  // loss; db2
    } else if (CH == 2) {
      s = bt::grad_entry<2>(p, params, [&](int c, int j, int k) { return totc(c, j * 7 + k); },
                            [&](int c, int j) { return (double)W2[c * H + j]; });
    } else {
      s = bt::grad_entry<1>(p, params, [&](int, int j, int k) { return tot(j * 7 + k); },
                            [&](int, int j) { return (double)W2[j]; });
    }
    if (p < P) slabA[(size_t)blockIdx.x * P + p] = s;
    else slabB[(size_t)blockIdx.x * 4 + 0] = s;
  }
  if (threadIdx.x < 3) slabB[(size_t)blockIdx.x * 4 + 1 + threadIdx.x] = 0.0;
}

// ---------------------------------------------------------------- launcher
bool launch_critic_step_v2(rl_traj *traj, const rl_mlp *critic, uint64_t B_total) {
  if (critic->general) return launch_gen_mfma(traj, critic, RL_GEN_CRITIC, nullptr, B_total, nullptr, 0.0f, 0.0f);
  if (!fused_5_128_fits(traj, critic, 1)) return false;  // (only feed-forward modules are passed here)
  traj_ensure_range(traj);
  const uint32_t *wimg = wimg_ensure(critic);
  ProfScope ps(traj->eng, RL_K_CRITIC_FUSED);
  float two_over_B = 2.0f / (float)B_total;
  traj->nbC = fused_grid(traj, CRITIC_WAVES);
  traj->last_rows = traj->nbC;
  const TrajDev d = fused_traj_dev(traj, traj->guard_next_critic);
  hipLaunchKernelGGL(k_critic_step_mfma<1>, dim3(traj->nbC), dim3(CRITIC_WAVES * 64), 0, traj->eng->stream, d,
                     critic->d_params, wimg, traj->slabA, traj->slabB, two_over_B, (uint32_t)critic->P,
                     bt::SHARE_OLD, bt::SHARE_YOUNG);  // (shares of the tiles: the kernel says why)
  return true;
}

// The DQN gradient of a 5-128-2 action-value network over the minibatch workspace `mb` (targets in `adv`, actions in
// `action`): k_critic_step_mfma<2>.  False: shape not built (the caller has other kernels).
bool launch_dqn_step_pair(rl_traj *mb, const rl_mlp *qnet, uint64_t B_total) {
  if (!fused_5_128_fits(mb, qnet, 2)) return false;  // (rl_dqn_create takes feed-forward modules only)
  const uint32_t *wimg = wimg_ensure(qnet);
  ProfScope ps(mb->eng, RL_K_POLICY_FUSED);
  // four tile-walking wave pairs per workgroup; slab rows of this launch (the slabs are sized for any grid up to 8 x CUs)
  mb->nbV2 = fused_grid(mb, CRITIC_WAVES / 2);
  TrajDev d = fused_traj_dev(mb, mb->guard_next_policy);
  d.tgt = mb->d.adv;  // (the minibatch workspace keeps its targets where a trajectory keeps advantages)
  hipLaunchKernelGGL(k_critic_step_mfma<2>, dim3(mb->nbV2), dim3(CRITIC_WAVES * 64), 0, mb->eng->stream, d,
                     qnet->d_params, wimg, mb->slabA, mb->slabB, 2.0f / (float)B_total, (uint32_t)qnet->P, 1u, 1u);
  RL_HIP_CHECK(hipGetLastError());
  return true;
}
