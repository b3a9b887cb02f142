// kernels_wide_split.hip — the update passes of a WIDE feed-forward module (rl_mlp_create_wide: 9 to 24 inputs) with ONE
// hidden layer of 65 to 128 units — the reference's default MlpConfig, hidden_sizes = [128] — as one fused launch per
// pass on v_mfma_f32_32x32x16_bf16.  kernels_wide_mfma.hip serves at most 64 units: as a one-wave kernel four unit
// tiles carry 144 accumulator registers and spill.  Here a 32-sample tile is shared by a TEAM of waves,
// each owning part of the hidden layer.
//
//   team        4 / OWN waves; wave h owns unit tiles h OWN .. h OWN + OWN - 1 of the hidden layer: their activations
//               and tangents, their deltas, their rows of dW_0 (the layer's bias is its column `in_dim`), their columns
//               of dW_o.  Wave 0 owns the output layer's bias column and counts the per-sample sums.  A workgroup holds
//               two teams: OWN = 1 is 512 threads, two waves per SIMD with 48 accumulator registers each.
//   layer 0     every wave loads the observation tile itself (wm_load_obs: straight from the feature-major planes into
//               the accumulator layout) and multiplies its truncated pieces against its own unit tiles' fragments
//               [ot][k-step][piece] of the LDS image (gm_build_image<false, 1, 4, 2>).  Nothing passes between waves.
//   output      each wave sums W_o (JVP: and the tangent's two terms) over its own units and leaves ZV floats per sample
//               in zbuf[parity][team][wave][ZV][32]; after ONE workgroup barrier every wave of the team adds the partial
//               sums in the same order — wave 0's, 1's, 2's, 3's, then the bias — so all hold bit-identical z, d0, d1.
//               The region is double-buffered by the parity of the iteration: a wave writes parity p again only behind
//               the barrier of the iteration between, which every wave passes after its reads of p.
//   backward    local to a wave: the per-sample terms (computed by every wave, identically), its own dl = W_o^T d, dW_o
//               and dW_0 = D_0 X^T through the on-pipe transposition, the observation tile loaded a second time.
//   tile walk   every team of a workgroup walks ceil(n_tiles / n_teams) iterations (the barrier is the workgroup's): a
//               team past the end runs on zeros.  One flush site, one slab row per team (its waves fill disjoint
//               entries), the scalar sums from wave 0.
// With one hidden layer there is no hidden-to-hidden product, so none of k_gen_pair's hand-overs of operand pieces.
#include "gen_mfma_common.hpp"

namespace {

constexpr int NL = 1, GW = 4;  // hidden layers, 32-unit tiles of the hidden layer
constexpr int WS_TEAMS = 2;    // teams of a workgroup
constexpr int WS_OWN = 1;      // unit tiles a wave owns: the instantiation that ships

// dynamic LDS: the weight image (PASS_JVP: the tangent's forward fragments beside the parameters'), then the partial
// output sums [2][WS_TEAMS][4 / OWN][ZV][32]
constexpr size_t ws_image_bytes(bool jvp) { return gm_image_bytes(false, GW, NL, jvp, WM_L0); }
constexpr size_t ws_lds_bytes(bool jvp, int own) { return ws_image_bytes(jvp) + (size_t)2 * WS_TEAMS * (4 / own) * (jvp ? 4 : 2) * 32 * 4; }
// (the index functions at GW = 4 with two k-steps of layer 0: forward layer 0 [4][2], forward output [8], backward output [4];
// the tangent's 16 forward groups behind them)
static_assert(gm_fo(GW, NL, WM_L0) == 8 && gm_bo(false, GW, NL, WM_L0) == 16 && gm_groups(false, GW, NL, WM_L0) == 20 &&
                  gm_all_groups(false, GW, NL, true, WM_L0) == 36,
              "k_wide_split: fragment groups");
static_assert(ws_image_bytes(false) == 61952 && ws_image_bytes(true) == 111616, "k_wide_split: image bytes");
static_assert(ws_lds_bytes(false, 1) == 66048 && ws_lds_bytes(true, 1) == 119808 && ws_lds_bytes(false, 2) == 64000 &&
                  ws_lds_bytes(true, 2) == 115712,
              "k_wide_split: LDS bytes");

template <int MODE, int OWN>
__global__ void __launch_bounds__(WS_TEAMS*(4 / OWN) * 64)
    k_wide_split(TrajDev tr, GmArgs g, float *__restrict__ lp0, double *__restrict__ slabA, double *__restrict__ slabB,
                 float inv_B, const int32_t *__restrict__ skip, float clip_lo, float clip_hi) {
  static_assert(OWN == 1 || OWN == 2, "a wave owns one or two unit tiles");
  extern __shared__ uint4 gm_lds[];
  uint4(*img)[64] = reinterpret_cast<uint4(*)[64]>(gm_lds);
  constexpr bool JVP = MODE == PASS_JVP, BWD = MODE != PASS_EVAL;
  constexpr int TW = 4 / OWN;                             // waves of a team
  constexpr int ZV = JVP ? 4 : 2;                         // partial outputs a wave hands over per sample
  constexpr int TG = gm_groups(false, GW, NL, WM_L0);     // first fragment group of the tangent parameters (JVP)
  constexpr int FO = gm_fo(GW, NL, WM_L0), BO = gm_bo(false, GW, NL, WM_L0);
  float *bias = reinterpret_cast<float *>(gm_lds + (size_t)gm_all_groups(false, GW, NL, JVP, WM_L0) * 3 * 64);  // [32 GW]: the outputs'
  float *tbias = bias + NL * 32 * GW;                                                                        // (JVP)
  float *zbuf = bias + NL * 32 * GW * (JVP ? 2 : 1);  // [2][WS_TEAMS][TW][ZV][32]
  if (skip != nullptr && *skip != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 31, kb = lane >> 5, team = wave / TW, h = wave % TW;

  gm_build_image<false, NL, GW, WM_L0>(g, g.params, img, 0, true, bias, WS_TEAMS * TW * 64);
  if (JVP) gm_build_image<false, NL, GW, WM_L0>(g, g.tangent, img, TG, false, tbias, WS_TEAMS * TW * 64);
  __syncthreads();

  Frag idb[2];
  bt::ident_frags(lane, idb);
  const f32x16 zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  // this wave's part of the weight gradients: layer 0 [o] (rows: its units; columns: the inputs, then the bias), output
  // [o] (rows: outputs; columns: its units), the output layer's bias (column 0 of the bias tile; wave 0 only)
  f32x16 dW0[OWN], dWo[OWN], dbt = zero16;
#pragma unroll
  for (int o = 0; o < OWN; ++o) {
    dW0[o] = zero16;
    dWo[o] = zero16;
  }
  double sum64[3] = {0.0, 0.0, 0.0};
  float sum32[3] = {0.0f, 0.0f, 0.0f};

  const size_t B = (size_t)tr.T * tr.n;
  const uint32_t B32 = (uint32_t)B, plane32 = (uint32_t)((size_t)(tr.T + 1) * tr.n);
  const size_t n_tiles = (B + 31) / 32;
  const size_t team_id = (size_t)blockIdx.x * WS_TEAMS + team, n_teams = (size_t)gridDim.x * WS_TEAMS;
  const size_t iters = (n_tiles + n_teams - 1) / n_teams;
  const GmLane w{m, kb, B32, plane32, n_tiles};
  GmRow row{slabA + team_id * g.P, true};  // the team's row
  auto flush_all = [&]() {
#pragma unroll
    for (int o = 0; o < OWN; ++o) gm_flush_w<NL>(g, row, m, kb, dW0[o], 0, h * OWN + o, 0);
#pragma unroll
    for (int o = 0; o < OWN; ++o) gm_flush_w<NL>(g, row, m, kb, dWo[o], NL, 0, h * OWN + o);
    gm_flush_rest<NL, GW>(g, row, m, kb, dbt, sum64, sum32, [&](int, int ot) { return ot == 0 && h == 0; });
  };

  int since_flush = 0;
  TileIn op = gm_load_tile<MODE, false>(tr, g, lp0, w, team_id);
  for (size_t it_ = 0; it_ < iters; ++it_) {
    const size_t t = team_id + it_ * n_teams;
    const TileIn next = gm_load_tile<MODE, false>(tr, g, lp0, w, t + n_teams);
    // ---- forward: this wave's unit tiles of layer 0 over both k-steps of the observation tile (JVP: the tangent rides
    // along, ta = act'(.) (V_0 x + vb_0))
    f32x16 a[OWN], ta[OWN];
    {
      const f32x16 x = wm_load_obs(tr, g, w, t);
      Frag xb0[WM_L0][3];
#pragma unroll
      for (int q = 0; q < WM_L0; ++q) pieces_trunc(x, q, xb0[q]);
#pragma unroll
      for (int o = 0; o < OWN; ++o) {
        f32x16 c = zero16;
#pragma unroll
        for (int q = 0; q < WM_L0; ++q) c = prod6_lds(c, img, (h * OWN + o) * WM_L0 + q, lane, xb0[q]);
        gm_act_tile(g.act, c);
        a[o] = c;
        if (JVP) {
          f32x16 tc = zero16;
#pragma unroll
          for (int q = 0; q < WM_L0; ++q) tc = prod6_lds(tc, img, TG + (h * OWN + o) * WM_L0 + q, lane, xb0[q]);
          gm_slope_tile(g.act, tc, c);
          ta[o] = tc;
        }
      }
    }
    // ---- output layer: the partial sums over this wave's units (rows 0 and 1 of the tile are the module's outputs)
    f32x16 zp = zero16, tzp = zero16;
#pragma unroll
    for (int o = 0; o < OWN; ++o)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int ks = (h * OWN + o) * 2 + q;
        Frag ab[3];
        pieces_trunc(a[o], q, ab);
        zp = prod6_lds(zp, img, FO + ks, lane, ab);
        if (JVP) {
          tzp = prod6_lds(tzp, img, TG + FO + ks, lane, ab);
          Frag tb[3];
          pieces_trunc(ta[o], q, tb);
          tzp = prod6_lds(tzp, img, FO + ks, lane, tb);
        }
      }
    float *zteam = zbuf + (((it_ & 1) * WS_TEAMS + team) * TW) * ZV * 32;
    if (kb == 0) {
      float *zmine = zteam + h * ZV * 32;
      zmine[m] = zp[0];
      zmine[32 + m] = zp[1];
      if (JVP) {
        zmine[64 + m] = tzp[0];
        zmine[96 + m] = tzp[1];
      }
    }
    __syncthreads();
    // (wave 0's part first, then 1, 2, 3, in every wave: all compute identical sums)
    auto meet = [&](int v, float b) {
      float s = zteam[v * 32 + m];
#pragma unroll
      for (int k = 1; k < TW; ++k) s = s + zteam[(k * ZV + v) * 32 + m];
      return s + b;
    };
    const float z0 = meet(0, bias[0]), z1 = meet(1, bias[1]);
    float tz0 = 0.0f, tz1 = 0.0f;
    if (JVP) {
      tz0 = meet(2, tbias[0]);
      tz1 = meet(3, tbias[1]);
    }
    // ---- per-sample terms: every wave computes them (identically), wave 0 of the team counts them
    float d0 = 0.0f, d1 = 0.0f;
    gm_sample_terms<MODE>(g, z0, z1, tz0, tz1, op, kb == 0 && op.valid, h == 0, inv_B, clip_lo, clip_hi, lp0,
                          (uint32_t)t * 32u + (uint32_t)m, B32, sum32, d0, d1);
    if (BWD) {
      // ---- output layer: its bias (wave 0), this wave's columns of dW_o, this wave's deltas dl = act'(.) W_o^T d
      Frag dob[1][3];
      gm_delta_pieces(d0, d1, kb, dob);
      Frag dT[2][3], aT[2][3];  // transposed pieces: the deltas in hand, the activations below them
      transpose_pieces<1>(dob, idb, dT);
      if (h == 0) dbt = bias_tile(dbt, dT, (NL - 1) * GW, m);
      f32x16 dl[OWN];
#pragma unroll
      for (int o = 0; o < OWN; ++o) {
        Frag ab[2][3];
#pragma unroll
        for (int q = 0; q < 2; ++q) pieces_trunc(a[o], q, ab[q]);
        transpose_pieces<2>(ab, idb, aT);
        dWo[o] = wgrad_tile(dWo[o], dT, aT);
        f32x16 c = prod6_lds(zero16, img, BO + h * OWN + o, lane, dob[0]);
        gm_slope_tile(g.act, c, a[o]);
        dl[o] = c;
      }
      // ---- layer 0: the observation tile (32 input rows: features, the bias input, zeros), transposed on the pipe,
      // against this wave's deltas
      {
        const f32x16 x = wm_load_obs(tr, g, w, t);
        Frag xb0[WM_L0][3];
#pragma unroll
        for (int q = 0; q < WM_L0; ++q) pieces_trunc(x, q, xb0[q]);
        transpose_pieces<WM_L0>(xb0, idb, aT);
      }
#pragma unroll
      for (int o = 0; o < OWN; ++o) {
        Frag db[2][3];
#pragma unroll
        for (int q = 0; q < 2; ++q) pieces_round(dl[o], q, db[q]);
        transpose_pieces<2>(db, idb, dT);
        dW0[o] = wgrad_tile(dW0[o], dT, aT);
      }
    }
    // one flush site: every GM_FLUSH tiles and after the last iteration
    if (++since_flush == GM_FLUSH || it_ + 1 == iters) {
      since_flush = 0;
      if (BWD) flush_all();
      else gm_fold(sum64, sum32);
    }
    op = next;
  }
  if (h != 0) return;  // the scalar sums live on wave 0 of the team
  gm_store_sums(sum64, kb, lane, slabB, team_id);
}

GmKernel ws_kernel_of(int mode) {
  if (mode == RL_GEN_CRITIC) return &k_wide_split<GM_CRITIC, WS_OWN>;
  if (mode == PASS_INIT) return &k_wide_split<PASS_INIT, WS_OWN>;
  if (mode == PASS_PPO) return &k_wide_split<PASS_PPO, WS_OWN>;
  if (mode == PASS_JVP) return &k_wide_split<PASS_JVP, WS_OWN>;
  return &k_wide_split<PASS_EVAL, WS_OWN>;
}

}  // namespace

// true when the passes of a wide module run as k_wide_split launches on the planes of `t`
bool wide_split_fits(const rl_traj *t, const rl_mlp *m) {
  if (!m->wide || !m->general || !m->has_bias || m->n_hidden != (uint32_t)NL) return false;
  if (m->widths[0] <= 64u || m->widths[0] > 32u * GW) return false;  // (at most 64 units: k_wide_mfma)
  if (m->in_dim > (uint32_t)WM_MAX_IN || m->out_dim > 2 || m->in_dim != t->d.D) return false;
  if ((uint64_t)(t->d.T + 1) * t->d.n * m->in_dim >= (1ull << 30)) return false;  // 32-bit element offsets in the kernel
  return true;
}

// mode: RL_GEN_CRITIC, PASS_INIT, PASS_PPO, PASS_EVAL or PASS_JVP (with the tangent parameters).  Leaves one slab row per
// team: t->last_rows rows of slabA (gradient modes) and slabB, and RL_PASS_PATH_WIDE_SPLIT in t->last_pass_path.
// false: shape not built.
bool launch_wide_split(rl_traj *t, const rl_mlp *m, int mode, const float *d_tangent, uint64_t B_total,
                       const int32_t *d_skip, float clip_lo, float clip_hi) {
  if (!wide_split_fits(t, m)) return false;
  if (mode != RL_GEN_CRITIC && mode != PASS_INIT && mode != PASS_PPO && mode != PASS_EVAL && mode != PASS_JVP) return false;
  if (mode == PASS_JVP && d_tangent == nullptr) return false;
  if (m->out_dim != (mode == RL_GEN_CRITIC ? 1u : 2u)) return false;
  GmArgs g{};
  g.params = m->d_params;
  g.tangent = d_tangent;
  g.in_dim = (int)m->in_dim;
  g.out_dim = (int)m->out_dim;
  g.act = m->act;
  g.out_act = m->out_act;
  for (uint32_t l = 0; l < m->n_hidden; ++l) g.width[l] = (int)m->widths[l];
  for (uint32_t l = 0; l <= m->n_hidden; ++l) g.off[l] = (uint32_t)m->layer_offset(l);
  g.P = (uint32_t)m->P;
  const uint64_t n_tiles = (t->B + 31) / 32, cus = (uint64_t)t->eng->prop.multiProcessorCount;
  const float inv_B = (mode == RL_GEN_CRITIC ? 2.0f : 1.0f) / (float)B_total;
  gen_ensure(t, m, 0, false, true);  // the P-sized vectors of the update workspace follow the module
  uint64_t nwg = (n_tiles + WS_TEAMS - 1) / WS_TEAMS;
  if (nwg > cus) nwg = cus;  // (the image leaves room for one workgroup per CU)
  t->last_rows = (uint32_t)(nwg * WS_TEAMS);  // every team flushes, the ones past the end zeros
  traj_ensure_slabs(t, t->last_rows, m->P, t->last_rows);
  gm_launch(ws_kernel_of(mode), t, g, (uint32_t)nwg, WS_TEAMS * (4 / WS_OWN) * 64, ws_lds_bytes(mode == PASS_JVP, WS_OWN), inv_B,
            d_skip, clip_lo, clip_hi);
  t->last_pass_path = RL_PASS_PATH_WIDE_SPLIT;
  return true;
}
