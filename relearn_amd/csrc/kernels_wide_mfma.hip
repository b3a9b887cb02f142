// kernels_wide_mfma.hip — the update passes of a WIDE feed-forward module (rl_mlp_create_wide: 9 to 24 inputs, the
// PartitionGame lanes' observation widths) as one fused launch per pass on v_mfma_f32_32x32x16_bf16: the
// gradient pass, the line search's evaluation, the Fisher-vector product and the PPO pass of a two-output policy, the
// regression step of a one-output critic.  kernels_gen_mfma.hip does this for at most seven inputs, and its layer 0 is
// where the bound comes from: it packs a sample's inputs (and the bias input) into ONE k-step of eight rows per lane half.
//
// What is shared with it (gen_mfma_common.hpp): hidden-layer chains with the tile's registers as B operand, exact
// three-piece products (six piece pairs), transposition on the pipe for the weight gradients, the bias column, the
// per-sample terms, and the tile walk, f32 -> f64 flush and epilogue of DESIGN 27.
//
// What is its own: layer 0 as a contraction over 32 padded input rows — two k-steps of 16 per piece pair.
//   observation tile   an ACCUMULATOR-layout tile, read straight from the trajectory's feature-major planes
//                      [D][(T + 1) n]: the sample on the lane (column lane & 31), the feature in the registers (row
//                      urow(r, lane >> 5)); register r of a half-wave loads 32 consecutive floats of one plane.  Row
//                      `in_dim` is the bias input (1); the rows above it, and the samples past B of the last tile, are
//                      zero and never touch memory.
//   forward            the tile, split into three bf16 pieces by truncation (exact, as the activations' split), is the
//                      B operand of Z_0^T = W_0 X^T against layer-0 weight fragments [out tile][k-step][piece] parked in
//                      LDS in the A-operand order (gm_build_image with L0 = 2: bias column `in_dim`).
//   weight gradient    dW_0 = D_0 X^T contracts over the samples: X goes through the on-pipe transposition the
//                      activation tiles go through, and one 32-unit x 32-input accumulator tile per output tile holds
//                      the (at most) 24 features and the bias column — the register count of the narrow kernel's layer 0.
// Shape: ONE hidden layer of at most 64 units (two 32-unit tiles), with bias vectors; one wave per SIMD, a tile of 32
// samples per wave and iteration.  The narrow kernel's other one-wave shapes — two layers of at most 64, one of at most
// 128 — carry 144 accumulator registers, and with layer 0's second k-step the compiler puts 256 to 476 bytes per lane
// of every gradient mode into scratch (profiles/wide_mlp_kernel_resources.json): they are not built here.
// One hidden layer of 65 to 128 units goes on to kernels_wide_split.hip, where a team of waves shares the tile (DESIGN
// 51); two-layer, three-layer and bias-less modules and planes of 2^30 elements run the per-layer kernels.
#include "gen_mfma_common.hpp"

namespace {

constexpr int NL = 1, GW = 2;  // hidden layers, 32-unit tiles of the hidden layer

// dynamic LDS: the weight image (PASS_JVP: the tangent's forward fragments beside the parameters')
constexpr size_t wm_lds_bytes(bool jvp) { return gm_image_bytes(false, GW, NL, jvp, WM_L0); }
static_assert(wm_lds_bytes(false) == 30976 && wm_lds_bytes(true) == 55808, "k_wide_mfma: LDS bytes");

template <int MODE>
__global__ void __launch_bounds__(GWAVES * 64)
    k_wide_mfma(TrajDev tr, GmArgs g, float *__restrict__ lp0, double *__restrict__ slabA, double *__restrict__ slabB,
                float inv_B, const int32_t *__restrict__ skip, float clip_lo, float clip_hi) {
  extern __shared__ uint4 gm_lds[];
  uint4(*img)[64] = reinterpret_cast<uint4(*)[64]>(gm_lds);
  constexpr bool JVP = MODE == PASS_JVP, BWD = MODE != PASS_EVAL;
  constexpr int TG = gm_groups(false, GW, NL, WM_L0);  // first fragment group of the tangent parameters (JVP)
  constexpr int FO = gm_fo(GW, NL, WM_L0), BO = gm_bo(false, GW, NL, WM_L0);
  float *bias = reinterpret_cast<float *>(gm_lds + (size_t)gm_all_groups(false, GW, NL, JVP, WM_L0) * 3 * 64);  // [NL][32 GW]
  float *tbias = bias + NL * 32 * GW;                                                                        // (JVP)
  if (skip != nullptr && *skip != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 31, kb = lane >> 5;

  gm_build_image<false, NL, GW, WM_L0>(g, g.params, img, 0, true, bias, GWAVES * 64);
  if (JVP) gm_build_image<false, NL, GW, WM_L0>(g, g.tangent, img, TG, false, tbias, GWAVES * 64);
  __syncthreads();

  Frag idb[2];
  bt::ident_frags(lane, idb);
  const f32x16 zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  // weight-gradient accumulators: layer 0 [ot] (columns: the inputs, then the bias), output [it] (rows:
  // outputs), the output layer's bias (column 0 of the bias tile)
  f32x16 dW0[GW], dWo[GW], dbt = zero16;
#pragma unroll
  for (int a = 0; a < GW; ++a) {
    dW0[a] = zero16;
    dWo[a] = zero16;
  }
  double sum64[3] = {0.0, 0.0, 0.0};
  float sum32[3] = {0.0f, 0.0f, 0.0f};

  const size_t B = (size_t)tr.T * tr.n;
  const uint32_t B32 = (uint32_t)B, plane32 = (uint32_t)((size_t)(tr.T + 1) * tr.n);
  const size_t n_tiles = (B + 31) / 32;
  const size_t wave_id = (size_t)blockIdx.x * GWAVES + wave, n_waves = (size_t)gridDim.x * GWAVES;
  if (wave_id >= n_tiles) return;  // (no barrier below; the launcher counts slab rows for the waves that have tiles)
  const GmLane w{m, kb, B32, plane32, n_tiles};
  GmRow row{slabA + wave_id * g.P, true};
  auto flush_all = [&]() {
#pragma unroll
    for (int ot = 0; ot < GW; ++ot) gm_flush_w<NL>(g, row, m, kb, dW0[ot], 0, ot, 0);
#pragma unroll
    for (int it = 0; it < GW; ++it) gm_flush_w<NL>(g, row, m, kb, dWo[it], NL, 0, it);
    gm_flush_rest<NL, GW>(g, row, m, kb, dbt, sum64, sum32, [](int l, int ot) { return ot >= 0 && ot < (l < NL ? GW : 1); });
  };
  auto bias_rows = [&](const float *table, int l, int ot) {  // accumulator initialised with the bias of its row's unit
    f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = table[(l - 1) * 32 * GW + ot * 32 + urow(r, kb)];
    return c;
  };

  int since_flush = 0;
  TileIn op = gm_load_tile<MODE, false>(tr, g, lp0, w, wave_id);
  for (size_t t = wave_id; t < n_tiles; t += n_waves) {
    const TileIn next = gm_load_tile<MODE, false>(tr, g, lp0, w, t + n_waves);
    // ---- forward: layer 0 over both k-steps of the observation tile (JVP: the tangent of every layer rides along,
    // ta_l = act'(.) (W_l ta_{l-1} + V_l a_{l-1} + vb_l), ta_{-1} = 0)
    f32x16 a[GW], ta[GW];
    {
      const f32x16 x = wm_load_obs(tr, g, w, t);
      Frag xb0[WM_L0][3];
#pragma unroll
      for (int q = 0; q < WM_L0; ++q) pieces_trunc(x, q, xb0[q]);
#pragma unroll
      for (int ot = 0; ot < GW; ++ot) {
        f32x16 c = zero16;
#pragma unroll
        for (int q = 0; q < WM_L0; ++q) c = prod6_lds(c, img, ot * WM_L0 + q, lane, xb0[q]);
        gm_act_tile(g.act, c);
        a[ot] = c;
        if (JVP) {
          f32x16 tc = zero16;
#pragma unroll
          for (int q = 0; q < WM_L0; ++q) tc = prod6_lds(tc, img, TG + ot * WM_L0 + q, lane, xb0[q]);
          gm_slope_tile(g.act, tc, c);
          ta[ot] = tc;
        }
      }
    }
    f32x16 zt = bias_rows(bias, NL, 0), tzt = zero16;
    {
      Frag ab[GW][2][3];
#pragma unroll
      for (int it = 0; it < GW; ++it)
#pragma unroll
        for (int q = 0; q < 2; ++q) pieces_trunc(a[it], q, ab[it][q]);
#pragma unroll
      for (int ks = 0; ks < 2 * GW; ++ks) zt = prod6_lds(zt, img, FO + ks, lane, ab[ks >> 1][ks & 1]);
      if (JVP) {
        tzt = bias_rows(tbias, NL, 0);
#pragma unroll
        for (int ks = 0; ks < 2 * GW; ++ks) {
          Frag tb[3];
          pieces_trunc(ta[ks >> 1], ks & 1, tb);
          tzt = prod6_lds(tzt, img, FO + ks, lane, tb);
          tzt = prod6_lds(tzt, img, TG + FO + ks, lane, ab[ks >> 1][ks & 1]);
        }
      }
    }
    // ---- per-sample terms on the lanes of half 0 (rows 0 and 1 of the output tile are the module's outputs)
    float d0 = 0.0f, d1 = 0.0f;
    gm_sample_terms<MODE>(g, zt[0], zt[1], tzt[0], tzt[1], op, kb == 0 && op.valid, true, inv_B, clip_lo, clip_hi, lp0,
                          (uint32_t)t * 32u + (uint32_t)m, B32, sum32, d0, d1);
    if (BWD) {
      // ---- output layer
      Frag dob[1][3];
      gm_delta_pieces(d0, d1, kb, dob);
      Frag dT[GW][2][3], aT[GW][2][3];  // transposed pieces: deltas of the layer in hand, activations below it
      transpose_pieces<1>(dob, idb, dT[0]);
      dbt = bias_tile(dbt, dT[0], (NL - 1) * GW, m);
      f32x16 dl[GW];  // deltas of the hidden layer in hand
#pragma unroll
      for (int it = 0; it < GW; ++it) {
        Frag ab[2][3];
#pragma unroll
        for (int q = 0; q < 2; ++q) pieces_trunc(a[it], q, ab[q]);
        transpose_pieces<2>(ab, idb, aT[it]);
        dWo[it] = wgrad_tile(dWo[it], dT[0], aT[it]);
        f32x16 c = prod6_lds(zero16, img, BO + it, lane, dob[0]);
        gm_slope_tile(g.act, c, a[it]);
        dl[it] = c;
      }
      // ---- layer 0: the observation tile (32 input rows: features, the bias input, zeros), transposed on the pipe,
      // against the deltas of hidden layer 0
      {
        const f32x16 x = wm_load_obs(tr, g, w, t);
        Frag xb0[WM_L0][3];
#pragma unroll
        for (int q = 0; q < WM_L0; ++q) pieces_trunc(x, q, xb0[q]);
        transpose_pieces<WM_L0>(xb0, idb, aT[0]);
      }
#pragma unroll
      for (int ot = 0; ot < GW; ++ot) {
        Frag db[2][3];
#pragma unroll
        for (int q = 0; q < 2; ++q) pieces_round(dl[ot], q, db[q]);
        transpose_pieces<2>(db, idb, dT[ot]);
        dW0[ot] = wgrad_tile(dW0[ot], dT[ot], aT[0]);
      }
    }
    // one flush site: every GM_FLUSH tiles and after the wave's last tile
    if (++since_flush == GM_FLUSH || t + n_waves >= n_tiles) {
      since_flush = 0;
      if (BWD) flush_all();
      else gm_fold(sum64, sum32);
    }
    op = next;
  }
  gm_store_sums(sum64, kb, lane, slabB, wave_id);
}

GmKernel wm_kernel_of(int mode) {
  if (mode == RL_GEN_CRITIC) return &k_wide_mfma<GM_CRITIC>;
  if (mode == PASS_INIT) return &k_wide_mfma<PASS_INIT>;
  if (mode == PASS_PPO) return &k_wide_mfma<PASS_PPO>;
  if (mode == PASS_JVP) return &k_wide_mfma<PASS_JVP>;
  return &k_wide_mfma<PASS_EVAL>;
}

}  // namespace

// true when the passes of a wide module run as fused matrix-pipe launches on the planes of `t`
bool wide_mfma_fits(const rl_traj *t, const rl_mlp *m) {
  if (!m->wide || !m->general || !m->has_bias || m->n_hidden != (uint32_t)NL || m->widths[0] > 32u * GW) return false;
  if (m->in_dim > (uint32_t)WM_MAX_IN || m->out_dim > 2 || m->in_dim != t->d.D) return false;
  if ((uint64_t)(t->d.T + 1) * t->d.n * m->in_dim >= (1ull << 30)) return false;  // 32-bit element offsets in the kernel
  return true;
}

// mode: RL_GEN_CRITIC, PASS_INIT, PASS_PPO, PASS_EVAL or PASS_JVP (with the tangent parameters).  Leaves one slab row per
// wave that has tiles: t->last_rows rows of slabA (gradient modes) and slabB.  false: shape not built.
bool launch_wide_mfma(rl_traj *t, const rl_mlp *m, int mode, const float *d_tangent, uint64_t B_total,
                      const int32_t *d_skip, float clip_lo, float clip_hi) {
  if (!wide_mfma_fits(t, m)) return false;
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
  uint64_t nwg = (n_tiles + GWAVES - 1) / GWAVES;
  if (nwg > cus) nwg = cus;
  t->last_rows = (uint32_t)(nwg * GWAVES < n_tiles ? nwg * GWAVES : n_tiles);
  traj_ensure_slabs(t, t->last_rows, m->P, t->last_rows);
  gm_launch(wm_kernel_of(mode), t, g, (uint32_t)nwg, GWAVES * 64, wm_lds_bytes(mode == PASS_JVP), inv_B,
            d_skip, clip_lo, clip_hi);
  return true;
}
