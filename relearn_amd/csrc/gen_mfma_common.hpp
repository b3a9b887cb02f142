// gen_mfma_common.hpp — what the fused matrix-pipe kernels of general MLPs share (kernels_gen_mfma.hip: at most seven
// inputs; kernels_wide_mfma.hip and kernels_wide_split.hip: 9 to 24): the LDS weight image and its index functions, the
// exact-piece products, the on-pipe transposition, the per-sample loss terms, and the tile walk, f32 -> f64 flush and
// epilogue of DESIGN 27.  Everything here has internal linkage: each of the units compiles its own copy.
#pragma once
#include <mutex>
#include <set>

#include "abi_internal.hpp"
#include "bf16_tile.hpp"
#include "device_fns.hpp"
#include "kernels.hpp"
#include "policy_fast.hpp"

namespace {

using bt::f32x16;
using bt::Frag;

constexpr int GWAVES = 4;      // waves per workgroup (one per SIMD, 512 registers each)
constexpr int GM_FLUSH = 64;   // f32 -> f64 flush period in tiles
constexpr int GM_MAX_HIDDEN = 3;

struct GmArgs {
  const float *params, *tangent;  // tangent: PASS_JVP only, laid out like params
  int in_dim, out_dim, act, out_act;
  int width[GM_MAX_HIDDEN];
  uint32_t off[GM_MAX_HIDDEN + 1];  // parameter offset of layer l's weights [N][K]; its bias follows them
  uint32_t P;
};
// fan-in and fan-out of layer l (layer NL: the output layer)
__device__ __forceinline__ int gm_K(const GmArgs &g, int l) { return l == 0 ? g.in_dim : g.width[l - 1]; }
template <int NL>
__device__ __forceinline__ int gm_N(const GmArgs &g, int l) { return l == NL ? g.out_dim : g.width[l]; }

// fragment groups of the LDS weight image (three piece fragments each): forward layer 0 [ot], forward hidden layer l
// [ot][ks], forward output [ks], backward hidden layer l [it][ks], backward output [it]
// (GW = 32-unit tiles per hidden layer: 2 for up to three layers of at most 64 units, 4 for one layer of at most 128)
// C, the COMPACT image of the pair kernel: the same groups without the output layer's forward fragments — of their 32
// rows only the module's (at most two) outputs are non-zero, so they live apart, behind the groups, one 16-byte entry per
// (k-step, piece, output, lane half) instead of 64: 1.5 KB instead of 12 KB (24 KB with the tangent's), which is what lets
// four pairs of waves and the tangent image share a CU's LDS.
// L0, the k-steps of layer 0: one (at most seven inputs and the bias input, packed by gm_input_pieces) or two (a wide
// module's 32 padded input rows, kernels_wide_mfma.hip: forward layer 0 [ot][k-step])
constexpr int gm_fh(int GW, int l, int L0 = 1) { return L0 * GW + (l - 1) * 2 * GW * GW; }
constexpr int gm_fo(int GW, int NL, int L0 = 1) { return L0 * GW + (NL - 1) * 2 * GW * GW; }
constexpr int gm_bh(bool C, int GW, int NL, int l, int L0 = 1) {
  return gm_fo(GW, NL, L0) + (C ? 0 : 2 * GW) + (l - 1) * 2 * GW * GW;
}
constexpr int gm_bo(bool C, int GW, int NL, int L0 = 1) { return gm_bh(C, GW, NL, NL, L0); }
constexpr int gm_groups(bool C, int GW, int NL, int L0 = 1) { return gm_bo(C, GW, NL, L0) + GW; }
// PASS_JVP: the forward fragments of the tangent parameters follow, in the same order (layer 0, hidden, output)
constexpr int gm_fwd_groups(bool C, int GW, int NL, int L0 = 1) { return gm_fo(GW, NL, L0) + (C ? 0 : 2 * GW); }
constexpr int gm_all_groups(bool C, int GW, int NL, bool jvp, int L0 = 1) {
  return gm_groups(C, GW, NL, L0) + (jvp ? gm_fwd_groups(C, GW, NL, L0) : 0);
}
constexpr int gm_outc_entries(int GW) { return 2 * GW * 3 * 4; }  // uint4 entries of one compact output-layer image
// the image in bytes: the groups, (C) the compact output fragments, the bias table [NL][32 GW] of layers 1 .. NL
constexpr size_t gm_image_bytes(bool C, int GW, int NL, bool jvp, int L0 = 1) {
  return (size_t)gm_all_groups(C, GW, NL, jvp, L0) * 3 * 64 * 16 + (C ? (size_t)(jvp ? 2 : 1) * gm_outc_entries(GW) * 16 : 0) +
         (size_t)NL * 32 * GW * 4 * (jvp ? 2 : 1);
}

__device__ __forceinline__ constexpr int urow(int r, int kb) { return (r & 3) + 8 * (r >> 2) + 4 * kb; }

__device__ __forceinline__ float gm_act(int act, float x) {
  if (act == RL_ACT_RELU) return __builtin_fmaxf(x, 0.0f);
  if (act == RL_ACT_SIGMOID) return fast_sigmoidf(x);
  if (act == RL_ACT_TANH) return fast_tanhf(x);
  return x;
}
__device__ __forceinline__ float gm_slope(int act, float y) {
  if (act == RL_ACT_RELU) return y > 0.0f ? 1.0f : 0.0f;
  if (act == RL_ACT_SIGMOID) return y * (1.0f - y);
  if (act == RL_ACT_TANH) return __builtin_fmaf(-y, y, 1.0f);
  return 1.0f;
}
// a whole tile at a time: one (wave-uniform) branch per tile, straight-line code inside
__device__ __forceinline__ void gm_act_tile(int act, f32x16 &c) {
  if (act == RL_ACT_RELU) {
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = __builtin_fmaxf(c[r], 0.0f);
  } else if (act == RL_ACT_SIGMOID) {
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = fast_sigmoidf(c[r]);
  } else if (act == RL_ACT_TANH) {
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = fast_tanhf(c[r]);
  }
}
// c *= act'(.) given the layer's outputs y
__device__ __forceinline__ void gm_slope_tile(int act, f32x16 &c, const f32x16 &y) {
  if (act == RL_ACT_RELU) {
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = y[r] > 0.0f ? c[r] : 0.0f;
  } else if (act == RL_ACT_SIGMOID) {
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = c[r] * (y[r] * (1.0f - y[r]));
  } else if (act == RL_ACT_TANH) {
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = c[r] * __builtin_fmaf(-y[r], y[r], 1.0f);
  }
}

// the B operand pieces of k-step q of an accumulator tile (registers 8 q .. 8 q + 7), by truncation (activations) ...
__device__ __forceinline__ void pieces_trunc(const f32x16 &t, int q, Frag (&x)[3]) {
  uint32_t p[3][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bt::split3t(t[8 * q + e], p[0][e], p[1][e], p[2][e]);
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) x[c].u[i] = bt::pkh(p[c][2 * i], p[c][2 * i + 1]);
}
// ... and by rounding (deltas)
__device__ __forceinline__ void pieces_round(const f32x16 &t, int q, Frag (&x)[3]) {
  uint32_t p[3][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bt::split3(t[8 * q + e], p[0][e], p[1][e], p[2][e]);
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) x[c].u[i] = bt::pk(p[c][2 * i], p[c][2 * i + 1]);
}

// acc += W X for one k-step: the six piece pairs that matter (w0 x0, w0 x1, w1 x0, w1 x1, w0 x2, w2 x0)
__device__ __forceinline__ f32x16 prod6(f32x16 acc, const Frag (&w)[3], const Frag (&x)[3]) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0].v, x[0].v, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0].v, x[1].v, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1].v, x[0].v, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1].v, x[1].v, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0].v, x[2].v, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[2].v, x[0].v, acc, 0, 0, 0);
  return acc;
}
__device__ __forceinline__ f32x16 prod6_lds(f32x16 acc, const uint4 (*img)[64], int grp, int lane, const Frag (&x)[3]) {
  Frag w[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) w[c].x = img[grp * 3 + c][lane];
  return prod6(acc, w, x);
}

// X^T of a tile given as packed pieces xb[q][piece] (k-steps q < QS): the pieces of X^T as operands of a product that
// sums over the SAMPLE, xt[sample k-step][piece]
template <int QS>
__device__ __forceinline__ void transpose_pieces(const Frag (&xb)[QS][3], const Frag (&idb)[2], Frag (&xt)[2][3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f32x16 d = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < QS; ++q) d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xb[q][c].v, idb[q].v, d, 0, 0, 0);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i) xt[s][c].u[i] = bt::pack_bf16(d[8 * s + 2 * i], d[8 * s + 2 * i + 1]);
  }
}

// dW += D^T-pieces x A^T-pieces over both sample k-steps
__device__ __forceinline__ f32x16 wgrad_tile(f32x16 acc, const Frag (&dt)[2][3], const Frag (&at)[2][3]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) acc = prod6(acc, dt[s], at[s]);
  return acc;
}
// bias column: sum over the samples of D^T's three pieces into column `c` of the bias tile
__device__ __forceinline__ f32x16 bias_tile(f32x16 acc, const Frag (&dt)[2][3], int c, int m) {
  Frag e;
  e.u[0] = e.u[1] = e.u[2] = e.u[3] = m == c ? 0x3F803F80u : 0u;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int p = 0; p < 3; ++p) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dt[s][p].v, e.v, acc, 0, 0, 0);
  return acc;
}

// ---- the weight image: every fragment in the acc_row order of the tile it meets.  `src`: the parameters (forward and
// backward fragments from group g0 = 0) or the tangent (forward fragments only, from group TG); every thread of the
// workgroup (`nthreads`) calls it, the caller synchronises.
// C: the compact layout (output-layer forward fragments into outc[(ks * 3 + piece) * 4 + 2 j + half]).
template <bool C, int NL, int GW, int L0 = 1>
__device__ __forceinline__ void gm_build_image(const GmArgs &g, const float *__restrict__ src, uint4 (*img)[64], int g0,
                                               bool with_backward, float *bias_out, int nthreads, uint4 *outc = nullptr) {
  auto put_group = [&](int grp, int ln, const float (&v)[8]) {
    uint32_t p[3][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bt::split3(v[e], p[0][e], p[1][e], p[2][e]);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      img[grp * 3 + c][ln] = make_uint4(bt::pk(p[c][0], p[c][1]), bt::pk(p[c][2], p[c][3]), bt::pk(p[c][4], p[c][5]),
                                        bt::pk(p[c][6], p[c][7]));
  };
  // forward, layer 0 [ot][k-step]: inputs 4 hh + e (e < 4) — L0 = 2: every row of both k-steps — the bias as input `in_dim`
  for (int idx = threadIdx.x; idx < L0 * GW * 64; idx += nthreads) {
    const int grp = idx >> 6, ot = grp / L0, ln = idx & 63, mm = ln & 31, hh = ln >> 5;
    const int unit = ot * 32 + mm, N = gm_N<NL>(g, 0);
    const float *W = src + g.off[0];
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = bt::acc_row(grp % L0, hh, e);
      v[e] = unit < N ? (k < g.in_dim ? W[unit * g.in_dim + k] : (k == g.in_dim ? W[N * g.in_dim + unit] : 0.0f)) : 0.0f;
    }
    put_group(g0 + grp, ln, v);
  }
  // forward [ot][ks] and backward [it][ks] through hidden layer l
#pragma unroll
  for (int l = 1; l < NL; ++l) {
    const int K = gm_K(g, l), N = gm_N<NL>(g, l);
    const float *W = src + g.off[l];
    for (int idx = threadIdx.x; idx < (with_backward ? 2 : 1) * 2 * GW * GW * 64; idx += nthreads) {
      const int dir = idx / (2 * GW * GW * 64), r2 = (idx >> 6) % (2 * GW * GW), ln = idx & 63, mm = ln & 31, hh = ln >> 5;
      const int tile = r2 / (2 * GW), ks = r2 % (2 * GW);
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int across = 32 * (ks >> 1) + bt::acc_row(ks & 1, hh, e), own = tile * 32 + mm;
        // forward: row = own output unit, column = input `across`; backward (W^T): row = own input, column = output
        const int j = dir == 0 ? own : across, k = dir == 0 ? across : own;
        v[e] = (j < N && k < K) ? W[j * K + k] : 0.0f;
      }
      put_group(g0 + (dir == 0 ? gm_fh(GW, l, L0) : gm_bh(C, GW, NL, l, L0)) + r2, ln, v);
    }
  }
  {  // output layer: forward [ks], backward [it]
    const int K = gm_K(g, NL);
    const float *W = src + g.off[NL];
    for (int idx = threadIdx.x; idx < (with_backward ? 3 : 2) * GW * 64; idx += nthreads) {
      const int q = idx >> 6, ln = idx & 63, mm = ln & 31, hh = ln >> 5;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        int j, k;
        if (q < 2 * GW) {
          j = mm;
          k = 32 * (q >> 1) + bt::acc_row(q & 1, hh, e);
        } else {
          j = bt::acc_row(0, hh, e);
          k = (q - 2 * GW) * 32 + mm;
        }
        v[e] = (j < g.out_dim && k < K) ? W[j * K + k] : 0.0f;
      }
      if (C && q < 2 * GW) {
        if (mm < 2) {
          uint32_t p[3][8];
#pragma unroll
          for (int e = 0; e < 8; ++e) bt::split3(v[e], p[0][e], p[1][e], p[2][e]);
#pragma unroll
          for (int c = 0; c < 3; ++c)
            outc[(q * 3 + c) * 4 + 2 * mm + hh] = make_uint4(bt::pk(p[c][0], p[c][1]), bt::pk(p[c][2], p[c][3]),
                                                             bt::pk(p[c][4], p[c][5]), bt::pk(p[c][6], p[c][7]));
        }
      } else {
        put_group(g0 + (q < 2 * GW ? gm_fo(GW, NL, L0) + q : gm_bo(C, GW, NL, L0) + (q - 2 * GW)), ln, v);
      }
    }
  }
#pragma unroll
  for (int l = 1; l <= NL; ++l) {
    const int N = gm_N<NL>(g, l), K = gm_K(g, l);
    for (int u = threadIdx.x; u < 32 * GW; u += nthreads) bias_out[(l - 1) * 32 * GW + u] = u < N ? src[g.off[l] + N * K + u] : 0.0f;
  }
}

constexpr int GM_CRITIC = 100;  // mean((V - target)^2); the policy modes are PASS_INIT / PASS_PPO / PASS_EVAL (kernels.hpp)

// one lane's view of a tile: its sample's inputs 4 kb .. 4 kb + 3 (bias input included) and per-sample scalars
struct TileIn {
  float x[4], tgt, adv, l0, l1;
  int act;
  bool valid;
};

// The per-sample loss terms from the module's two (pre-activation) outputs z0, z1 (JVP: and their tangents):
// d0 / d1 = d loss / d (pre-activation of output 0 / 1) on `owner` lanes, the pass's scalar sums on lanes that `counts`
// (the arithmetic of k_policy_bf16's per-sample section, kernels_mfma.hip; critic: mean((V - target)^2), inv_B = 2 / B).
template <int MODE>
__device__ __forceinline__ void gm_sample_terms(const GmArgs &g, float z0, float z1, float tz0, float tz1, const TileIn &op,
                                                bool owner, bool counts, float inv_B, float clip_lo, float clip_hi,
                                                float *__restrict__ lp0, uint32_t sidx, uint32_t B32, float (&sum32)[3],
                                                float &d0, float &d1) {
  constexpr bool JVP = MODE == PASS_JVP;
  if (MODE == GM_CRITIC) {
    const float v = gm_act(g.out_act, z0);
    const float d = v - op.tgt;
    if (owner) {
      if (counts) sum32[0] = __builtin_fmaf(d, d, sum32[0]);
      d0 = d * inv_B * gm_slope(g.out_act, v);  // inv_B = 2 / B here
    }
  } else if (JVP) {
    // Fisher metric of the categorical head on the tangent outputs: dz_a = p_a (ty_a - sum_b p_b ty_b) / B; two
    // actions: dz_0 = -dz_1 = p_0 p_1 (ty_0 - ty_1) / B
    const float y0 = gm_act(g.out_act, z0), y1 = gm_act(g.out_act, z1);
    const float s0 = gm_slope(g.out_act, y0), s1 = gm_slope(g.out_act, y1);
    const SoftPair sp = soft_pair(y0 - y1);
    const float gz = (sp.p[0] * sp.p[1]) * (tz0 * s0 - tz1 * s1) * inv_B;
    if (owner) {
      d0 = gz * s0;
      d1 = -gz * s1;
    }
  } else {
    const float y0 = gm_act(g.out_act, z0), y1 = gm_act(g.out_act, z1);
    const SoftPair sp = soft_pair(y0 - y1);
    const float adv = op.adv;
    const int act = op.act;
    const float lpa = act == 0 ? sp.lp[0] : sp.lp[1];
    float g0 = 0.0f, g1 = 0.0f;  // d loss / d output
    if (MODE == PASS_INIT) {
      if (owner && counts) {
        lp0[sidx] = sp.lp[0];
        lp0[B32 + sidx] = sp.lp[1];
      }
      const float cc = -adv * inv_B;  // ratio = exp(lpa - lpa) = 1
      g0 = cc * ((act == 0 ? 1.0f : 0.0f) - sp.p[0]);
      g1 = cc * ((act == 1 ? 1.0f : 0.0f) - sp.p[1]);
      const float cl0 = sp.lp[0] < -3.402823466e+38f ? -3.402823466e+38f : sp.lp[0];
      const float cl1 = sp.lp[1] < -3.402823466e+38f ? -3.402823466e+38f : sp.lp[1];
      float ent = cl0 * sp.p[0];
      ent += cl1 * sp.p[1];
      if (owner && counts) {
        sum32[0] = sum32[0] + adv;  // ratio * adv
        sum32[1] = sum32[1] - ent;
        sum32[2] = __builtin_fmaf(lpa, adv, sum32[2]);
      }
    } else if (MODE == PASS_PPO) {
      // clipped surrogate (policies/ppo.rs:124-137); see k_policy_pass for the tie rules of minimum()/clamp()
      const float l0a = act == 0 ? op.l0 : op.l1;
      const float ratio = fast_expf(lpa - l0a);
      const float clipped = ratio < clip_lo ? clip_lo : (ratio > clip_hi ? clip_hi : ratio);
      const float u1 = ratio * adv, u2 = clipped * adv;
      const bool inside = ratio >= clip_lo && ratio <= clip_hi;
      const float gr = u1 < u2 ? adv : (u1 > u2 ? (inside ? adv : 0.0f) : (inside ? adv : 0.5f * adv));
      const float cc = -(gr * ratio) * inv_B;
      g0 = cc * ((act == 0 ? 1.0f : 0.0f) - sp.p[0]);
      g1 = cc * ((act == 1 ? 1.0f : 0.0f) - sp.p[1]);
      if (owner && counts) sum32[0] = sum32[0] + (u1 < u2 ? u1 : u2);
    } else {  // PASS_EVAL: surrogate and KL(pi_0 || pi) of candidate parameters
      const float l0a = act == 0 ? op.l0 : op.l1;
      const float ratio = fast_expf(lpa - l0a);
      float rel0 = op.l0 - sp.lp[0], rel1 = op.l1 - sp.lp[1];
      if (rel0 < -3.402823466e+38f) rel0 = -3.402823466e+38f;
      if (rel1 < -3.402823466e+38f) rel1 = -3.402823466e+38f;
      const SoftPair old = soft_pair(op.l0 - op.l1);
      float kl = rel0 * old.p[0];
      kl += rel1 * old.p[1];
      if (owner && counts) {
        sum32[0] = __builtin_fmaf(ratio, adv, sum32[0]);
        sum32[1] = sum32[1] + kl;
      }
    }
    if (owner) {
      d0 = g0 * gm_slope(g.out_act, y0);
      d1 = g1 * gm_slope(g.out_act, y1);
    }
  }
}

// ================================================================================================
// What the two kernels below share around their chains.  Each keeps its accumulator set, its forward, backward
// and weight-gradient chains and its assignment of tiles to waves.
// ================================================================================================
// a lane's place in the walk: its sample column and register half, the sample and tile counts
struct GmLane {
  int m, kb;
  uint32_t B32, plane32;
  size_t n_tiles;
};

// the operands of tile t (branch-free: padding lanes, and every lane of a tile past the last, read sample B - 1 and are
// zeroed)
// (INPUTS false: the per-sample scalars alone — a wide module's observation tile is loaded by its own kernel)
template <int MODE, bool INPUTS = true>
__device__ __forceinline__ TileIn gm_load_tile(const TrajDev &tr, const GmArgs &g, const float *lp0, const GmLane &w, size_t t) {
  TileIn o;
  const uint32_t sidx = (uint32_t)t * 32u + (uint32_t)w.m;
  o.valid = t < w.n_tiles && sidx < w.B32;
  const uint32_t sc = o.valid ? sidx : w.B32 - 1;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = 4 * w.kb + e;
    float v = 0.0f;
    if (INPUTS && k < g.in_dim) v = tr.obs[(uint32_t)k * w.plane32 + sc];
    else if (INPUTS && k == g.in_dim) v = 1.0f;
    o.x[e] = o.valid ? v : 0.0f;
  }
  o.tgt = o.adv = o.l0 = o.l1 = 0.0f;
  o.act = 0;
  if (MODE == GM_CRITIC) {
    const float tg = tr.tgt[sc];
    o.tgt = o.valid ? tg : 0.0f;
  } else if (MODE != PASS_JVP) {
    const float adv = tr.adv[sc];
    const int act = (int)tr.action[sc];
    o.adv = o.valid ? adv : 0.0f;
    o.act = o.valid ? act : 0;
    if (MODE != PASS_INIT) {
      const float l0 = lp0[sc], l1 = lp0[w.B32 + sc];
      o.l0 = o.valid ? l0 : 0.0f;
      o.l1 = o.valid ? l1 : 0.0f;
    }
  }
  return o;
}

// ---- layer 0 of a wide module (kernels_wide_mfma.hip, kernels_wide_split.hip): 32 padded input rows
constexpr int WM_L0 = 2;  // k-steps of layer 0
constexpr int WM_MAX_IN = 24;
// the observation tile of tile t: feature urow(r, kb) of the lane's sample in register r.  The kernel reads it twice, for
// the forward and again (from the cache) for layer 0's weight gradient, instead of keeping its 16 registers — or its 24
// of packed pieces — alive across the tile's chains.  (The lane's column
// through a register the optimiser cannot see through, or the two reads become one value that lives across the tile.)
__device__ __forceinline__ f32x16 wm_load_obs(const TrajDev &tr, const GmArgs &g, const GmLane &w, size_t t) {
  int mo = w.m;
  asm volatile("" : "+v"(mo));
  const uint32_t sidx = (uint32_t)t * 32u + (uint32_t)mo;
  const bool valid = t < w.n_tiles && sidx < w.B32;
  f32x16 x;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int k = urow(r, w.kb);
    float v = 0.0f;
    if (valid) {
      if (k < g.in_dim) v = tr.obs[(uint32_t)k * w.plane32 + sidx];
      else if (k == g.in_dim) v = 1.0f;
    }
    x[r] = v;
  }
  return x;
}

// the B operand pieces of the input tile: the lane's four inputs (bias input included), by truncation
__device__ __forceinline__ void gm_input_pieces(const TileIn &op, Frag (&xb0)[1][3]) {
  uint32_t p[3][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) bt::split3t(op.x[e], p[0][e], p[1][e], p[2][e]);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    xb0[0][c].u[0] = bt::pkh(p[c][0], p[c][1]);
    xb0[0][c].u[1] = bt::pkh(p[c][2], p[c][3]);
    xb0[0][c].u[2] = xb0[0][c].u[3] = 0u;
  }
}
// ... and of the output layer's deltas (units 0 and 1 = elements 0 and 1 of half 0's k-step 0), by rounding
__device__ __forceinline__ void gm_delta_pieces(float d0, float d1, int kb, Frag (&dob)[1][3]) {
  uint32_t p0[3], p1[3];
  bt::split3(d0, p0[0], p0[1], p0[2]);
  bt::split3(d1, p1[0], p1[1], p1[2]);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    dob[0][c].u[0] = kb == 0 ? bt::pk(p0[c], p1[c]) : 0u;
    dob[0][c].u[1] = dob[0][c].u[2] = dob[0][c].u[3] = 0u;
  }
}

// The slab row of a wave, or of a pair (its two waves fill disjoint entries): one f64 entry per parameter.
struct GmRow {
  double *p;
  bool first;  // nothing flushed yet: an entry is stored, not added to
  __device__ __forceinline__ void put(uint32_t at, float v) const {
    if (first) p[at] = (double)v;
    else p[at] = p[at] + (double)v;
  }
};
// slab entry += tile entry for the valid (output j, input k) of weight tile (ot, it) of layer l (layer 0: and its bias,
// the input behind the last); the tile is cleared
template <int NL>
__device__ __forceinline__ void gm_flush_w(const GmArgs &g, const GmRow &row, int m, int kb, f32x16 &t, int l, int ot, int it) {
  // (the lane's column through a register the optimiser cannot see through: with a visible one, the ~100 slab addresses
  // and bounds of a flush are loop-invariant, get computed ahead of the tile loop and live in scratch until the flush —
  // ~1 KB per lane written and read back by every launch: 270 MB at 16,384 x 128 samples)
  int mo = m, kbo = kb;
  asm volatile("" : "+v"(mo), "+v"(kbo));
  const int K = gm_K(g, l), N = gm_N<NL>(g, l), k = it * 32 + mo;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int j = ot * 32 + urow(r, kbo);
    if (j < N) {
      if (k < K) row.put(g.off[l] + (uint32_t)(j * K + k), t[r]);
      else if (l == 0 && k == K) row.put(g.off[0] + (uint32_t)(N * K + j), t[r]);
    }
    t[r] = 0.0f;
  }
  // (the slab updates of one tile at a time: hoisting every load of the flush above the first store needs ~400 more
  // registers than the kernel has)
  __builtin_amdgcn_sched_barrier(0);
}
// f32 -> f64 fold of the scalar sums
__device__ __forceinline__ void gm_fold(double (&sum64)[3], float (&sum32)[3]) {
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    sum64[q] += (double)sum32[q];
    sum32[q] = 0.0f;
  }
}
// the rest of a flush, behind the weight tiles: the biases of layers 1 .. NL — column c = (l - 1) GW + ot of the bias
// tile, flushed by the wave that owns(l, ot) — and the scalar sums
template <int NL, int GW, class Owns>
__device__ __forceinline__ void gm_flush_rest(const GmArgs &g, GmRow &row, int m, int kb, f32x16 &dbt, double (&sum64)[3],
                                              float (&sum32)[3], Owns owns) {
#pragma unroll
  for (int l = 1; l <= NL; ++l) {
    int mo = m, kbo = kb;
    asm volatile("" : "+v"(mo), "+v"(kbo));  // (as in gm_flush_w)
    const int N = gm_N<NL>(g, l), K = gm_K(g, l), ot = mo - (l - 1) * GW;
    if (owns(l, ot)) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = ot * 32 + urow(r, kbo);
        if (j < N) row.put(g.off[l] + (uint32_t)(N * K + j), dbt[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) dbt[r] = 0.0f;
  gm_fold(sum64, sum32);
  row.first = false;
}
// the scalar sums of a walk: over the wave's 32 owner lanes, into row `id` of slabB
__device__ __forceinline__ void gm_store_sums(double (&sum64)[3], int kb, int lane, double *slabB, size_t id) {
#pragma unroll
  for (int q = 0; q < 3; ++q) sum64[q] = bt::owner_sum(sum64[q], kb);
  if (lane == 0) {
    double *sb = slabB + id * 4;
    sb[0] = sum64[0];
    sb[1] = sum64[1];
    sb[2] = sum64[2];
    sb[3] = 0.0;
  }
}

using GmKernel = void (*)(TrajDev, GmArgs, float *, double *, double *, float, const int32_t *, float, float);

// one launch; the kernel's dynamic LDS limit is raised once per device and kernel
void gm_launch(GmKernel kernel, rl_traj *t, const GmArgs &g, uint32_t nwg, uint32_t threads, size_t lds, float inv_B,
               const int32_t *d_skip, float clip_lo, float clip_hi) {
  {
    static std::mutex mu;
    static std::set<std::pair<GmKernel, int>> raised;
    std::lock_guard<std::mutex> lock(mu);
    if (raised.insert({kernel, t->eng->device}).second)
      RL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  hipLaunchKernelGGL(kernel, dim3(nwg), dim3(threads), lds, t->eng->stream, t->d, g, t->lp0, t->slabA, t->slabB, inv_B, d_skip,
                     clip_lo, clip_hi);
  RL_HIP_CHECK(hipGetLastError());
}

}  // namespace
