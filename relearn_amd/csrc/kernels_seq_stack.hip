// kernels_seq_stack.hip — recurrent chains with RnnBaseConfig::num_layers > 1 (src/torch/modules/seq/rnn/mod.rs:20-45,
// 223-257): stacked GRU / LSTM layers -> ReLU -> Mlp([h]) (modules/chain.rs:127-186).  Flat order per layer
// [W_ih (gates x layer input), W_hh (gates x hidden), b_ih, b_hh]; layer 0 reads the observation features, layer l > 0
// the hidden output of layer l - 1 of the same step (Tensor::gru / ::lstm with num_layers, seq/rnn/gru.rs:41-66); no
// dropout.  Every layer's state is zero at t = 0 and after a step whose flag ends the episode.  The chain's second
// module is a compile-time parameter of every kernel (LIN): the Mlp([h]) above, or one Linear(H, A) on relu(top)
// (ChainConfig<_, LinearConfig>, modules/chain.rs:12-54; flat order [.., kernel [A][H], bias [A]]): no hidden units,
// so no `u` / `ur` / `du` planes and one barrier less per step.  So is the head's output-count class (NQ): 2 for the
// chains of one or two outputs, 4 or 8 for the chains of rl_rnn_chain_create over IndexSpace::new(3..8), 12 for those of
// rl_rnn_chain_create_wide over 9..12, whose outputs are computed in passes of four rows (head_passes).
//
// The single-layer chains have fused tile kernels (kernels_seq*.hip, built for 5 -> 128 -> 128); this is the general
// path for the stacked ones, at the module's own widths: ONE THREAD PER LANE, 64 lanes per workgroup, and the unit loop
// of a layer dealt in quads to the workgroup's eight waves (a quad's gate rows share every loaded input value: 12-16 fma
// per load; weights come through wave-uniform loads).  States and the step's scratch live in [unit][lane] arrays in
// device memory (L2-resident: a workgroup's slice is 64 lanes wide), records of a training forward in [unit][sample]
// planes — the layout the per-layer weight-gradient kernel of kernels_general.hip reads, which forms every dW = dY X^T
// here as well.  Arithmetic contract of the forward: acc = bias; acc = fma(in_k, w_k, acc), k ascending, and the cells'
// operation order of seq_common.hpp — the tests' C restatement follows the same contract, so outputs compare bit for
// bit; backward and tangent passes are checked against an f64 restatement to f32 tolerance.
//   k_stack_forward   teacher-forced forward over T steps (+ successor outputs of cut episodes, + the record)
//   k_stack_step      one rollout step from the env's observation buffer (states persist between the launches)
//   k_stack_rollout   all T rollout steps of an env's lanes in one launch (the env's ops struct is a template argument)
//   k_stack_backward  reverse scan: d loss / d pre-activations of every layer and of the head into planes
//   k_stack_tangent   forward-mode derivative along a parameter tangent through the recorded activations
#include "abi_internal.hpp"
#include "device_fns.hpp"
#include "dqn_lanes.hpp"
#include "env_lanes.hpp"

namespace {

constexpr int SL = 64;  // lanes per workgroup
constexpr int SW = 8;   // waves per workgroup
constexpr int UQ = 4;   // units per pass (forward-style products: the quad's gate rows share every loaded input)
constexpr int KB = 8;   // outputs per pass of the transposed products of the backward scan
constexpr int LSTM = RL_MODULE_LSTM_MLP, GRU = RL_MODULE_GRU_MLP;

// record planes of a layer: [RPN][H][B]
enum { RP_G0 = 0, RP_G1 = 1, RP_G2 = 2, RP_G3 = 3, RP_HPREV = 4, RP_HOUT = 5, RP_CPREV = 6, RP_TC = 7, RPN = 8 };
// state sets (h at slot 2 s, c at 2 s + 1)
enum { SET_A = 0, SET_B = 1, SET_PEEK = 2, SET_TA = 3, SET_TB = 4, N_SETS = 5 };

struct StackNet {
  const float *p;  // flat parameters (or a tangent in the same layout)
  const float *z;  // >= 4 H zeros: what a layer WITHOUT bias vectors starts its gate rows from (NULL: the layers have them)
  int D, H, H2, A, L;
  uint32_t off[RL_RNN_MAX_LAYERS + 1];  // W_ih of layer l; [L]: the head's W1 (linear tail: its kernel; H2 is 0)
};
// How a kernel reads the module's parameters.  CW false: through the plain pointer (the compiler takes wave-uniform
// scalar loads where it can prove that no store of the kernel reaches the load: k_stack_step).  CW true: through the
// constant address space — the parameters are not written while a kernel of this unit runs, and a kernel that loops over
// the steps with stores of its own in the loop keeps the scalar loads only when told so (k_stack_rollout: without it the
// weights came through 120 per-lane vector loads instead of 87 scalar ones).
template <bool CW>
struct WeightPtr {
  using type = const float *;
};
template <>
struct WeightPtr<true> {
  using type = const __attribute__((address_space(4))) float *;
};
template <bool CW>
__device__ __forceinline__ typename WeightPtr<CW>::type weight_ptr(const float *p) {
  return (typename WeightPtr<CW>::type)p;
}

// b_ih / b_hh of a layer whose W_hh starts at Whh
template <int G>
__device__ __forceinline__ const float *stack_bih(const StackNet &net, const float *Whh) {
  return net.z != nullptr ? net.z : Whh + (size_t)G * net.H * net.H;
}
template <int G>
__device__ __forceinline__ const float *stack_bhh(const StackNet &net, const float *Whh) {
  return net.z != nullptr ? net.z : Whh + (size_t)G * net.H * net.H + G * net.H;
}

struct StackWs {
  float *st, *u, *din, *dst, *rec, *a1, *ur, *dg, *du;
  uint32_t n;
  uint64_t B;
};

template <int CELL>
__host__ __device__ constexpr int gates() { return CELL == LSTM ? 4 : 3; }

__device__ __forceinline__ float *slot(const StackWs &ws, const StackNet &net, int set, int hc, int l) {
  return ws.st + (((size_t)(2 * set + hc) * net.L + l) * net.H) * ws.n;
}
__device__ __forceinline__ float *rec_plane(const StackWs &ws, const StackNet &net, int l, int which) {
  return ws.rec + (((size_t)l * RPN + which) * net.H) * ws.B;
}

struct LaneCtx {
  uint32_t ii;  // lane (clamped into range: threads past n compute along and store nothing)
  bool live;
  int wave;
};

__device__ __forceinline__ LaneCtx lane_ctx(uint32_t n) {
  LaneCtx c;
  const uint32_t i = blockIdx.x * SL + (threadIdx.x & (SL - 1));
  c.live = i < n;
  c.ii = c.live ? i : n - 1;
  c.wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  return c;
}

// acc[r] = fma(x_k, W[row[r]][k], acc[r]) for k ascending: R rows of a [.][K] matrix against one input vector.  Four k
// per trip: a row's four weights are contiguous (one wide wave-uniform load each), the four inputs are in flight
// together; every sum stays the k-ascending fma chain of the arithmetic contract.
template <int R, class WP, class XF>
__device__ __forceinline__ void dot_rows(float (&acc)[R], WP W, const int (&row)[R], int K, XF x_at) {
  int k = 0;
  for (; k + 4 <= K; k += 4) {
    float x[4], w[R][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = x_at(k + q);
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) w[r][q] = W[(size_t)row[r] * K + k + q];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = __builtin_fmaf(x[q], w[r][q], acc[r]);
  }
  for (; k < K; ++k) {
    const float x = x_at(k);
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = __builtin_fmaf(x, W[(size_t)row[r] * K + k], acc[r]);
  }
}

// acc[u] += sum over r < R of d_r W[r][k0 + u]: N outputs k0 .. k0 + N - 1 of the transposed product W^T d (W rows `ld`
// floats apart).  FULL: all N outputs exist (contiguous weights, wide loads); else indices past kmax are clamped.
template <int N, bool FULL, class DF>
__device__ __forceinline__ void tdot_n(float (&acc)[N], const float *__restrict__ W, int ld, int k0, int kmax, int R,
                                       DF d_at) {
  int kk[N];
#pragma unroll
  for (int u = 0; u < N; ++u) kk[u] = FULL ? k0 + u : (k0 + u < kmax ? k0 + u : kmax);
  int r = 0;
  for (; r + 4 <= R; r += 4) {
    float d[4], w[4][N];
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q] = d_at(r + q);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int u = 0; u < N; ++u) w[q][u] = W[(size_t)(r + q) * ld + kk[u]];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int u = 0; u < N; ++u) acc[u] = __builtin_fmaf(d[q], w[q][u], acc[u]);
  }
  for (; r < R; ++r) {
    const float d = d_at(r);
#pragma unroll
    for (int u = 0; u < N; ++u) acc[u] = __builtin_fmaf(d, W[(size_t)r * ld + kk[u]], acc[u]);
  }
}
template <int N, class DF>
__device__ __forceinline__ void tdot(float (&acc)[N], const float *__restrict__ W, int ld, int k0, int K, int R, DF d_at) {
  if (k0 + N <= K) tdot_n<N, true>(acc, W, ld, k0, K - 1, R, d_at);
  else tdot_n<N, false>(acc, W, ld, k0, K - 1, R, d_at);
}

// The head's outputs of a module with more than two of them (rl_rnn_chain_create, out_dim 3..8;
// rl_rnn_chain_create_wide, 9..12), NQ registers of a thread (4, 8 or 12): passes of UQ output rows, every output the
// contract's chain — acc = bias[q]; acc = fma(x_k, w[q][k], acc), k ascending — from `bias_at(q)` through `dots(acc, rows)`, which runs one dot_rows per matrix of the sum.  Rows
// past A repeat row A - 1 (never stored); a pass wholly past A is skipped (A is wave-uniform).
template <int NQ, class BF, class DF>
__device__ __forceinline__ void head_passes(float (&out)[NQ], int A, BF bias_at, DF dots) {
  static_assert(NQ % UQ == 0, "whole passes");
#pragma unroll
  for (int q0 = 0; q0 < NQ; q0 += UQ) {
    float acc[UQ] = {};
    if (q0 < A) {
      int qq[UQ];
#pragma unroll
      for (int u = 0; u < UQ; ++u) {
        qq[u] = q0 + u < A ? q0 + u : A - 1;
        acc[u] = bias_at(qq[u]);
      }
      dots(acc, qq);
    }
#pragma unroll
    for (int u = 0; u < UQ; ++u) out[q0 + u] = acc[u];
  }
}
// dst[q][b] = o[q] (or 0 where `take` is false) for the module's A outputs, planes `stride` apart.  NQ > 2: the
// register array is indexed by the unrolled loop only (a run-time index would put it in scratch).
template <int NQ>
__device__ __forceinline__ void store_outputs(float *__restrict__ dst, size_t stride, size_t b, const float (&o)[NQ],
                                              int A, bool take) {
  if constexpr (NQ == 2) {
    for (int q = 0; q < A; ++q) dst[(size_t)q * stride + b] = take ? o[q] : 0.0f;
  } else {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (q < A) dst[(size_t)q * stride + b] = take ? o[q] : 0.0f;
  }
}

// layer l of one step: in[k * in_stride + lane] (K inputs), states (h, c) -> (hn, cn); `fresh`: the lane's state is zero
// HOLD (the DQN collection, k_stack_collect_dqn): a lane with `hold` set passes its state through, bit for bit — (hn, cn)
// = (h, c), zero where `fresh` — whatever the step computed for it
template <int CELL, bool REC, bool CW = false, bool HOLD = false>
__device__ __forceinline__ void stack_cell(const StackNet &net, const StackWs &ws, int l, const float *__restrict__ in,
                                           size_t in_stride, const float *__restrict__ h, const float *__restrict__ c,
                                           bool fresh, float *__restrict__ hn, float *__restrict__ cn, const LaneCtx &lc,
                                           size_t b, bool hold = false) {
  constexpr int G = gates<CELL>();
  const int H = net.H, K = l == 0 ? net.D : net.H;
  const size_t n = ws.n;
  const float *__restrict__ Wih_p = net.p + net.off[l], *__restrict__ Whh_p = Wih_p + (size_t)G * H * K;
  const auto Wih = weight_ptr<CW>(Wih_p), Whh = weight_ptr<CW>(Whh_p);
  const auto bih = weight_ptr<CW>(stack_bih<G>(net, Whh_p)), bhh = weight_ptr<CW>(stack_bhh<G>(net, Whh_p));
  for (int j0 = UQ * lc.wave; j0 < H; j0 += UQ * SW) {
    float gif[G * UQ], ghf[G * UQ];  // [gate][unit of the quad]
    int row[G * UQ];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int u = 0; u < UQ; ++u) {
        const int j = j0 + u < H ? j0 + u : H - 1;
        row[g * UQ + u] = g * H + j;
        gif[g * UQ + u] = bih[g * H + j];
        ghf[g * UQ + u] = bhh[g * H + j];
      }
    dot_rows(gif, Wih, row, K, [&](int k) { return in[(size_t)k * in_stride + lc.ii]; });
    dot_rows(ghf, Whh, row, H, [&](int k) { return fresh ? 0.0f : h[(size_t)k * n + lc.ii]; });
    float gi[G][UQ], gh[G][UQ];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int u = 0; u < UQ; ++u) {
        gi[g][u] = gif[g * UQ + u];
        gh[g][u] = ghf[g * UQ + u];
      }
#pragma unroll
    for (int u = 0; u < UQ; ++u) {
      const int j = j0 + u;
      if (j >= H) break;
      const float hp = fresh ? 0.0f : h[(size_t)j * n + lc.ii];
      float hnew;
      if (CELL == LSTM) {
        const float cp = fresh ? 0.0f : c[(size_t)j * n + lc.ii];
        const float ig = rl_sigmoidf(gh[0][u] + gi[0][u]), fg = rl_sigmoidf(gh[1][u] + gi[1][u]);
        const float gg = rl_tanhf(gh[2][u] + gi[2][u]), og = rl_sigmoidf(gh[G - 1][u] + gi[G - 1][u]);
        const float fc = fg * cp;
        const float iga = ig * gg;
        const float cc = fc + iga;
        const float tc = rl_tanhf(cc);
        hnew = og * tc;
        if (lc.live) {
          cn[(size_t)j * n + lc.ii] = HOLD && hold ? cp : cc;
          if (REC) {
            rec_plane(ws, net, l, RP_G0)[(size_t)j * ws.B + b] = ig;
            rec_plane(ws, net, l, RP_G1)[(size_t)j * ws.B + b] = fg;
            rec_plane(ws, net, l, RP_G2)[(size_t)j * ws.B + b] = gg;
            rec_plane(ws, net, l, RP_G3)[(size_t)j * ws.B + b] = og;
            rec_plane(ws, net, l, RP_CPREV)[(size_t)j * ws.B + b] = cp;
            rec_plane(ws, net, l, RP_TC)[(size_t)j * ws.B + b] = tc;
          }
        }
      } else {
        const float r = rl_sigmoidf(gh[0][u] + gi[0][u]);
        const float z = rl_sigmoidf(gh[1][u] + gi[1][u]);
        const float rn = gh[2][u] * r;
        const float nn = rl_tanhf(gi[2][u] + rn);
        const float dn = hp - nn;
        const float hz = dn * z;
        hnew = hz + nn;
        if (REC && lc.live) {
          rec_plane(ws, net, l, RP_G0)[(size_t)j * ws.B + b] = r;
          rec_plane(ws, net, l, RP_G1)[(size_t)j * ws.B + b] = z;
          rec_plane(ws, net, l, RP_G2)[(size_t)j * ws.B + b] = nn;
          rec_plane(ws, net, l, RP_G3)[(size_t)j * ws.B + b] = gh[2][u];
        }
      }
      if (HOLD && hold) hnew = hp;
      if (lc.live) {
        hn[(size_t)j * n + lc.ii] = hnew;
        if (REC) {
          rec_plane(ws, net, l, RP_HPREV)[(size_t)j * ws.B + b] = hp;
          rec_plane(ws, net, l, RP_HOUT)[(size_t)j * ws.B + b] = hnew;
        }
      }
    }
  }
}

// Chain's ReLU and the Mlp on the top layer's output `top` ([H][n]); out[q] in every thread.  One barrier inside.
// LIN: Chain's ReLU and one Linear — out[q] = bias[q] + sum_k relu(top[k]) kernel[q][k], no barrier.
// NQ: the output-count class — 2 for the chains of one or two outputs, 4, 8 or 12 for more (head_passes).
template <bool REC, bool CW = false, bool LIN = false, int NQ = 2>
__device__ __forceinline__ void stack_head(const StackNet &net, const StackWs &ws, const float *__restrict__ top,
                                           const LaneCtx &lc, size_t b, float (&out)[NQ]) {
  const int H = net.H, H2 = net.H2, A = net.A;
  const size_t n = ws.n;
  if (LIN) {
    const float *__restrict__ Wk_p = net.p + net.off[net.L], *__restrict__ bk_p = Wk_p + (size_t)A * H;
    const auto Wk = weight_ptr<CW>(Wk_p), bk = weight_ptr<CW>(bk_p);
    if (REC && lc.live)
      for (int k = lc.wave; k < H; k += SW) {
        const float tv = top[(size_t)k * n + lc.ii];
        ws.a1[(size_t)k * ws.B + b] = tv > 0.0f ? tv : 0.0f;
      }
    auto relu_top = [&](int k) {
      const float tv = top[(size_t)k * n + lc.ii];
      return tv > 0.0f ? tv : 0.0f;
    };
    if constexpr (NQ == 2) {
      const int qq[2] = {0, A > 1 ? 1 : 0};
      out[0] = bk[qq[0]];
      out[1] = bk[qq[1]];
      dot_rows(out, Wk, qq, H, relu_top);
    } else {
      head_passes(out, A, [&](int q) { return bk[q]; },
                  [&](float (&acc)[UQ], const int (&qq)[UQ]) { dot_rows(acc, Wk, qq, H, relu_top); });
    }
    return;
  }
  const float *__restrict__ W1_p = net.p + net.off[net.L], *__restrict__ b1_p = W1_p + (size_t)H2 * H;
  const float *__restrict__ W2_p = b1_p + H2, *__restrict__ b2_p = W2_p + (size_t)A * H2;
  const auto W1 = weight_ptr<CW>(W1_p), b1 = weight_ptr<CW>(b1_p), W2 = weight_ptr<CW>(W2_p), b2 = weight_ptr<CW>(b2_p);
  for (int j0 = UQ * lc.wave; j0 < H2; j0 += UQ * SW) {
    float acc[UQ];
    int jj[UQ];
#pragma unroll
    for (int u = 0; u < UQ; ++u) {
      jj[u] = j0 + u < H2 ? j0 + u : H2 - 1;
      acc[u] = b1[jj[u]];
    }
    dot_rows(acc, W1, jj, H, [&](int k) {
      const float tv = top[(size_t)k * n + lc.ii];
      return tv > 0.0f ? tv : 0.0f;
    });
#pragma unroll
    for (int u = 0; u < UQ; ++u)
      if (j0 + u < H2 && lc.live) {
        const float uu = acc[u] > 0.0f ? acc[u] : 0.0f;
        ws.u[(size_t)(j0 + u) * n + lc.ii] = uu;
        if (REC) ws.ur[(size_t)(j0 + u) * ws.B + b] = uu;
      }
  }
  if (REC && lc.live)
    for (int k = lc.wave; k < H; k += SW) {
      const float tv = top[(size_t)k * n + lc.ii];
      ws.a1[(size_t)k * ws.B + b] = tv > 0.0f ? tv : 0.0f;
    }
  __syncthreads();
  auto unit = [&](int j) { return ws.u[(size_t)j * n + lc.ii]; };
  if constexpr (NQ == 2) {
    const int qq[2] = {0, A > 1 ? 1 : 0};
    out[0] = b2[qq[0]];
    out[1] = b2[qq[1]];
    dot_rows(out, W2, qq, H2, unit);
  } else {
    head_passes(out, A, [&](int q) { return b2[q]; },
                [&](float (&acc)[UQ], const int (&qq)[UQ]) { dot_rows(acc, W2, qq, H2, unit); });
  }
}

// all layers + head of one step: states of set `cur` (zero where `fresh`) -> set `nxt`
// (HOLD / hold: stack_cell's; the outputs of a held lane are not its action values and are not to be used)
template <int CELL, bool REC, bool CW = false, bool LIN = false, int NQ = 2, bool HOLD = false>
__device__ __forceinline__ void stack_module_step(const StackNet &net, const StackWs &ws, const float *__restrict__ x,
                                                  size_t x_stride, int cur, int nxt, bool fresh, const LaneCtx &lc,
                                                  size_t b, float (&out)[NQ], bool hold = false) {
  for (int l = 0; l < net.L; ++l) {
    const float *in = l == 0 ? x : slot(ws, net, nxt, 0, l - 1);
    stack_cell<CELL, REC, CW, HOLD>(net, ws, l, in, l == 0 ? x_stride : (size_t)ws.n, slot(ws, net, cur, 0, l),
                                    slot(ws, net, cur, 1, l), fresh, slot(ws, net, nxt, 0, l), slot(ws, net, nxt, 1, l),
                                    lc, b, hold);
    __syncthreads();
  }
  stack_head<REC, CW, LIN, NQ>(net, ws, slot(ws, net, nxt, 0, net.L - 1), lc, b, out);
}

// teacher-forced forward: out / succ [A][T][n] (succ may be NULL), the contract of launch_gru_seq_forward
template <int CELL, bool REC, bool LIN = false, int NQ = 2>
__global__ void __launch_bounds__(SL *SW) k_stack_forward(StackNet net, StackWs ws, TrajDev tr, float *__restrict__ out,
                                                          float *__restrict__ succ, const int32_t *__restrict__ skip) {
  if (skip != nullptr && *skip != 0) return;
  const LaneCtx lc = lane_ctx(tr.n);
  const size_t n = tr.n, T = tr.T, B = T * n, plane = (T + 1) * n;
  bool fresh = true;
  int cur = SET_A;
  for (size_t t = 0; t < T; ++t) {
    const size_t b = t * n + lc.ii;
    float o[NQ];
    stack_module_step<CELL, REC, false, LIN, NQ>(net, ws, tr.obs + t * n, plane, cur, cur ^ 1, fresh, lc, b, o);
    const uint8_t f = tr.flag[b];
    if (lc.live && lc.wave == 0) store_outputs(out, B, b, o, net.A, true);
    if (succ != nullptr) {
      const bool need = f == RL_SUCC_INTERRUPT || (f == RL_SUCC_CONTINUE && t == T - 1);
      float o2[NQ] = {};
      if (__syncthreads_or(need && lc.live ? 1 : 0)) {
        // the successor observation (the interrupted step's, or obs[T] at the horizon) evaluated from the states after
        // step t, which are not advanced: the results go to the third state set.  Per-lane plane stride: term_obs planes
        // are T * n apart, obs planes (T + 1) * n.
        const bool intr = f == RL_SUCC_INTERRUPT;
        stack_module_step<CELL, false, false, LIN, NQ>(net, ws, intr ? tr.term_obs + t * n : tr.obs + T * n,
                                                       intr ? B : plane, cur ^ 1, SET_PEEK, false, lc, b, o2);
      }
      if (lc.live && lc.wave == 0) store_outputs(succ, B, b, o2, net.A, need);
    }
    fresh = f != RL_SUCC_CONTINUE;
    cur ^= 1;
  }
}

// one rollout step: env observation buffer obs [D][n] -> logits z [A][n]; the lane's states restart where the step
// before ended its episode (flag_prev: that step's successor codes) or at the first step of a collection
template <int CELL, bool LIN = false, int NQ = 2>
__global__ void __launch_bounds__(SL *SW) k_stack_step(StackNet net, StackWs ws, const float *__restrict__ obs,
                                                       const uint8_t *__restrict__ flag_prev, int first, int parity,
                                                       float *__restrict__ z) {
  const LaneCtx lc = lane_ctx(ws.n);
  const bool fresh = first != 0 || flag_prev[lc.ii] != RL_SUCC_CONTINUE;
  float o[NQ];
  stack_module_step<CELL, false, false, LIN, NQ>(net, ws, obs, (size_t)ws.n, parity, parity ^ 1, fresh, lc, 0, o);
  if constexpr (NQ == 2) {
    if (lc.live && lc.wave == 0)
      for (int q = 0; q < net.A; ++q) z[(size_t)q * ws.n + lc.ii] = o[q];
  } else {
    if (lc.live && lc.wave == 0) store_outputs(z, (size_t)ws.n, (size_t)lc.ii, o, net.A, true);
  }
}

// All T steps of a rollout in one launch: what launch_rollout_stepwise's five launches per step (record the observation,
// k_stack_step, PolicyActor::act, the env's step kernel, record the step) compute, value for value.  A workgroup keeps
// its 64 lanes for the whole horizon and nothing crosses workgroups, so a step needs barriers only.  Per step: the
// module reads the observation from the trajectory's planes (slot t, written by wave 0 one step earlier — plane stride
// (T + 1) n as in k_stack_forward); the lane's wave-0 thread draws the action from word t_global + t of the lane's actor
// stream with k_gen_sample_actions<NA>'s code (NA: the env's action count = the module's outputs), steps the lane (lane_step, TrajSink) and writes the features of the next
// observation into slot t + 1 (slot T after the last step); a barrier publishes them and the successor codes, from
// which every thread of the lane learns whether the states restart (k_stack_step's flag_prev).  Lane state lives in wave
// 0's registers from the first step to the last.
template <int CELL, class Env, int D, bool LIN = false, int NA = 2>
__global__ void __launch_bounds__(SL *SW) k_stack_rollout(StackNet net, StackWs ws, CartPoleDev c, EnvStateDev st,
                                                          TrajDev tr, uint64_t t_global) {
  __shared__ uint8_t succ_of[SL];
  constexpr int NQ = NA <= 2 ? 2 : ((NA + UQ - 1) / UQ) * UQ;
  const LaneCtx lc = lane_ctx(tr.n);
  const size_t n = tr.n, T = tr.T, plane = (T + 1) * n;
  const bool actor = lc.wave == 0, writer = lc.live && actor;
  const uint64_t glane = c.lane_offset + lc.ii;
  typename Env::State s{};
  if (actor) {
    Env::load(st, lc.ii, s);
    float f[D];
    Env::template features<D>(c, s, f);
    if (writer) {
#pragma unroll
      for (int d = 0; d < D; ++d) tr.obs[d * plane + lc.ii] = f[d];
    }
  }
  __syncthreads();
  bool fresh = true;
  int cur = SET_A;
  for (size_t t = 0; t < T; ++t) {
    float o[NQ];
    stack_module_step<CELL, false, true, LIN, NQ>(net, ws, tr.obs + t * n, plane, cur, cur ^ 1, fresh, lc, 0, o);
    if (actor) {
      const float u = rl_u32_to_unit_f32(stream_word(c.key_actor, glane, t_global + t));
      float lp[NA];
      if constexpr (NA == 2) {
        log_softmax_lane<2>(o, lp);
      } else {
        float zz[NA];
#pragma unroll
        for (int q = 0; q < NA; ++q) zz[q] = o[q];
        log_softmax_lane<NA>(zz, lp);
      }
      const int a = categorical_sample_lane<NA>(lp, u);
      TrajSink sink{tr, t * n + lc.ii, writer};
      float f[D];
      const int succ = lane_step<Env, D>(c, s, a, glane, t_global + t, sink, f);
      Env::template features<D>(c, s, f);
      if (writer) {
#pragma unroll
        for (int d = 0; d < D; ++d) tr.obs[d * plane + (t + 1) * n + lc.ii] = f[d];
      }
      succ_of[threadIdx.x] = (uint8_t)succ;  // (wave 0: threadIdx.x < SL)
    }
    __syncthreads();
    fresh = succ_of[threadIdx.x & (SL - 1)] != RL_SUCC_CONTINUE;
    cur ^= 1;
  }
  if (writer) Env::store(st, lc.ii, s);
}

// All T collection steps of a DQN agent with a recurrent action-value module in one launch (rl_dqn_create_recurrent):
// k_stack_rollout's module step joined with k_rollout_dqn's actor and replay ring (kernels_dqn.hip, dqn_lanes.hpp).
// DqnActor::act (dqn.rs:360-379) draws gen_bool(eps) first and, when the step explores, returns gen_range(0..NA) BEFORE
// the module's step(): the module never sees that observation and the lane's recurrent state is what it was.  Per step:
//   wave 0   the lane's observation features -> the observation planes `xobs` ([D][.][n], plane stride `xstride`); the
//            exploration draw and, for an exploring lane, the random action; the decision -> LDS
//   barrier  (also the vote: a workgroup whose lanes all explore skips the module step — nothing is advanced, and the
//            state sets are not swapped)
//   all      the module step, exploring lanes held (stack_cell HOLD: their states pass through bit for bit)
//   wave 0   the greedy action (first maximal index), Env::step, the ring record (+ `hi` for D > 5, the successor
//            observation of an Interrupt, flags_out), the horizon rule and the auto-reset of k_rollout_dqn; the successor
//            code -> LDS
//   barrier  every thread of the lane learns whether its state is zero at the next step: after an episode's end, or
//            still — a lane that has only explored since
// The lane's env state, ring words and LaneActorRng live in wave 0's registers from the first step to the last; the
// state is zero at the first step of every launch (the ring closes a lane the horizon cuts as Interrupt: what follows is
// a new recorded episode).  A lane whose ring refuses a step (WriteExperienceError::Full) stops acting and follows the
// barriers; the host raises the error.
// NA: the env's action count = the module's outputs (rl_dqn_create_finite: 3..8), taken as in k_stack_rollout — the head
// computes NQ outputs in passes of four rows, the greedy action is the first maximal of the first NA.
template <int CELL, class Env, int D, bool LIN, int NA = 2>
__global__ void __launch_bounds__(SL *SW) k_stack_collect_dqn(StackNet net, StackWs ws, CartPoleDev c, EnvStateDev st,
                                                              ReplayDev rp, float *__restrict__ xobs, size_t xstride,
                                                              uint32_t T, uint64_t p_int, int always_explore,
                                                              uint8_t *__restrict__ flags_out, uint64_t t_global) {
  __shared__ uint32_t words[16 * SL];  // LaneActorRng's block columns (wave 0)
  __shared__ uint8_t succ_of[SL], hold_of[SL];
  constexpr int NQ = NA <= 2 ? 2 : ((NA + UQ - 1) / UQ) * UQ;
  const uint32_t n = rp.N;
  const LaneCtx lc = lane_ctx(n);
  const bool actor = lc.wave == 0, writer = lc.live && actor;
  const uint32_t col = threadIdx.x & (SL - 1);
  const uint64_t glane = c.lane_offset + lc.ii;
  typename Env::State s{};
  LaneRing ring{};
  LaneEpEnds eps{rp.ep_end, n, lc.ii, writer};
  LaneActorRng<SL> rng{&words[col], c.key_actor, glane, 0, ~0ull};
  if (actor) {
    Env::load(st, lc.ii, s);
    ring = ring_load(rp, lc.ii);
    rng.pos = rp.actor_pos[lc.ii];
  }
  bool fresh = true, full = false;
  int cur = SET_A;
  for (uint32_t t = 0; t < T; ++t) {
    float f[D];
    bool explore = true;
    int a = 0;
    if (actor) {
      Env::template features<D>(c, s, f);
      if (!full) {
        explore = dqn_explores(rng, p_int, always_explore);
        if (explore) a = dqn_random_action<NA>(rng);
      }
      if (writer && !explore) {
#pragma unroll
        for (int d = 0; d < D; ++d) xobs[(size_t)d * xstride + lc.ii] = f[d];
      }
      hold_of[col] = explore ? 1 : 0;
    }
    const int any_greedy = __syncthreads_or(writer && !explore ? 1 : 0);
    const bool hold = hold_of[col] != 0;
    float o[NQ] = {};
    if (any_greedy) {
      stack_module_step<CELL, false, true, LIN, NQ, true>(net, ws, xobs, xstride, cur, cur ^ 1, fresh, lc, 0, o, hold);
      cur ^= 1;
    }
    if (actor) {
      int succ = RL_SUCC_CONTINUE;
      if (!full) {
        if (!explore) {  // argmax: first maximal index
          if constexpr (NA == 2) {
            a = o[1] > o[0] ? 1 : 0;
          } else {
            float zz[NA];
#pragma unroll
            for (int q = 0; q < NA; ++q) zz[q] = o[q];
            a = first_max_index<NA>(zz);
          }
        }
        float reward;
        succ = Env::step(c, s, a, glane, t_global + t, reward);
        const bool horizon_cut = succ == RL_SUCC_CONTINUE && t + 1 == T;
        const int succ_rec = horizon_cut ? RL_SUCC_INTERRUPT : succ;
        const uint32_t slot_abs = ring_write_step(ring, rp.C, rp.E, eps, succ_rec != RL_SUCC_CONTINUE);
        if (slot_abs == 0xffffffffu) {
          full = true;  // WriteExperienceError::Full: a single episode longer than the lane's capacity
          succ = RL_SUCC_CONTINUE;
        } else {
          const size_t o_rec = (size_t)lc.ii * rp.C + slot_abs % rp.C;
          if (writer) {
            ReplayRec rec;
#pragma unroll
            for (int d = 0; d < 5; ++d) rec.x[d] = d < D ? f[d < D ? d : 0] : 0.0f;
            rec.reward = reward;
            rec.af = (uint32_t)a | (uint32_t)succ_rec << 8;
            rec_store(rp.rec + o_rec, rec);
            if constexpr (D > 5)
              rp.hi[o_rec] = make_float4(f[5], D > 6 ? f[D > 6 ? 6 : 0] : 0.0f, D > 7 ? f[D > 7 ? 7 : 0] : 0.0f, 0.0f);
          }
          if (succ_rec == RL_SUCC_INTERRUPT) {
            Env::template features<D>(c, s, f);
            if (writer) {
#pragma unroll
              for (int d = 0; d < D; ++d) rp.next[o_rec].x[d] = f[d];
            }
          }
          if (writer) flags_out[(size_t)t * n + lc.ii] = (uint8_t)succ_rec;
          if (succ != RL_SUCC_CONTINUE) Env::reset(c, s, glane);
        }
      }
      succ_of[col] = (uint8_t)succ;
    }
    __syncthreads();
    fresh = succ_of[col] != RL_SUCC_CONTINUE || (hold && fresh);
  }
  if (!writer) return;
  if (full) *rp.error = 1;
  ring_store(rp, lc.ii, ring);
  rp.actor_pos[lc.ii] = rng.pos;
  Env::store(st, lc.ii, s);
}

// Reverse scan over the record of the last training forward: dz [A][B] -> d loss / d pre-activation planes
//   du [H2][B]   the head's hidden layer
//   dg [L][4H][B] the layers' gates — GRU rows [r; z; n (input side); n (hidden side, x r)], LSTM rows [i; f; g; o]
// from which the weight-gradient kernel forms every dW / db.  Per step and layer: (A) this wave's units turn the gradient
// into their output (carried from step t + 1, zero across an episode boundary, plus what the layer above — or the head —
// sends down at this step) into gate deltas; (B) this wave's input indices k gather W_hh^T / W_ih^T times those deltas:
// the gradient carried to step t - 1 and the one sent to the layer below.  LIN: no du plane, the head is one
// transposed product, din[k] = [top[k] > 0] sum_q kernel[q][k] dz[q].
template <int CELL, bool LIN = false>
__global__ void __launch_bounds__(SL *SW) k_stack_backward(StackNet net, StackWs ws, TrajDev tr,
                                                           const float *__restrict__ dz,
                                                           const int32_t *__restrict__ skip) {
  if (skip != nullptr && *skip != 0) return;
  constexpr int G = gates<CELL>();
  const LaneCtx lc = lane_ctx(tr.n);
  const size_t n = tr.n, T = tr.T, B = T * n;
  const int H = net.H, H2 = net.H2, A = net.A, L = net.L;
  const float *__restrict__ W1 = net.p + net.off[L], *__restrict__ W2 = W1 + (size_t)H2 * H + H2;
  for (size_t t = T; t-- > 0;) {
    const size_t b = t * n + lc.ii;
    const bool ended = t == T - 1 || tr.flag[b] != RL_SUCC_CONTINUE;  // nothing flows in from step t + 1
    if (!LIN) {
      for (int j0 = KB * lc.wave; j0 < H2; j0 += KB * SW) {
        float acc[KB] = {};
        tdot(acc, W2, H2, j0, H2, A, [&](int q) { return dz[(size_t)q * B + b]; });
#pragma unroll
        for (int u = 0; u < KB; ++u)
          if (j0 + u < H2 && lc.live)
            ws.du[(size_t)(j0 + u) * B + b] = ws.ur[(size_t)(j0 + u) * B + b] > 0.0f ? acc[u] : 0.0f;
      }
      __syncthreads();
    }
    {
      // (LIN: W1 is the Linear's kernel [A][H], and dz is what comes down)
      const float *__restrict__ top = rec_plane(ws, net, L - 1, RP_HOUT);
      for (int k0 = KB * lc.wave; k0 < H; k0 += KB * SW) {
        float acc[KB] = {};
        tdot(acc, W1, H, k0, H, LIN ? A : H2,
             [&](int j) { return LIN ? dz[(size_t)j * B + b] : ws.du[(size_t)j * B + b]; });
#pragma unroll
        for (int u = 0; u < KB; ++u)
          if (k0 + u < H && lc.live)
            ws.din[(size_t)(k0 + u) * n + lc.ii] = top[(size_t)(k0 + u) * B + b] > 0.0f ? acc[u] : 0.0f;
      }
    }
    __syncthreads();
    for (int l = L - 1; l >= 0; --l) {
      const int K = l == 0 ? net.D : H;
      const float *__restrict__ Wih = net.p + net.off[l], *__restrict__ Whh = Wih + (size_t)G * H * K;
      float *__restrict__ dhc = ws.dst + ((size_t)l * H) * n, *__restrict__ dcc = ws.dst + ((size_t)(L + l) * H) * n;
      float *__restrict__ dg = ws.dg + ((size_t)l * 4 * H) * B;
      // (A)
      for (int j0 = UQ * lc.wave; j0 < H; j0 += UQ * SW)
#pragma unroll
        for (int u = 0; u < UQ; ++u) {
          const int j = j0 + u;
          if (j >= H) break;
          const size_t jb = (size_t)j * B + b, jn = (size_t)j * n + lc.ii;
          const float dhl = (ended ? 0.0f : dhc[jn]) + ws.din[jn];
          if (CELL == LSTM) {
            const float ig = rec_plane(ws, net, l, RP_G0)[jb], fg = rec_plane(ws, net, l, RP_G1)[jb];
            const float gg = rec_plane(ws, net, l, RP_G2)[jb], og = rec_plane(ws, net, l, RP_G3)[jb];
            const float cp = rec_plane(ws, net, l, RP_CPREV)[jb], tc = rec_plane(ws, net, l, RP_TC)[jb];
            const float dO = dhl * tc;
            const float dcn = (ended ? 0.0f : dcc[jn]) + dhl * og * (1.0f - tc * tc);
            if (lc.live) {
              dg[jb] = dcn * gg * ig * (1.0f - ig);
              dg[(size_t)H * B + jb] = dcn * cp * fg * (1.0f - fg);
              dg[(size_t)2 * H * B + jb] = dcn * ig * (1.0f - gg * gg);
              dg[(size_t)3 * H * B + jb] = dO * og * (1.0f - og);
              dcc[jn] = dcn * fg;
              dhc[jn] = 0.0f;
            }
          } else {
            const float r = rec_plane(ws, net, l, RP_G0)[jb], z = rec_plane(ws, net, l, RP_G1)[jb];
            const float nn = rec_plane(ws, net, l, RP_G2)[jb], ghn = rec_plane(ws, net, l, RP_G3)[jb];
            const float hp = rec_plane(ws, net, l, RP_HPREV)[jb];
            const float dzg = dhl * (hp - nn);
            const float dn = dhl * (1.0f - z);
            const float dpn = dn * (1.0f - nn * nn);
            const float dr = dpn * ghn;
            if (lc.live) {
              dg[jb] = dr * r * (1.0f - r);
              dg[(size_t)H * B + jb] = dzg * z * (1.0f - z);
              dg[(size_t)2 * H * B + jb] = dpn;
              dg[(size_t)3 * H * B + jb] = dpn * r;
              dhc[jn] = dhl * z;  // h' = (h - n) z + n: the direct path
            }
          }
        }
      __syncthreads();
      // (B)
      for (int k0 = KB * lc.wave; k0 < H; k0 += KB * SW) {
        float acc[KB] = {}, acc2[KB] = {};
        // hidden-side delta of gate row `row`: the GRU's n rows take their fourth plane
        tdot(acc, Whh, H, k0, H, G * H, [&](int row) {
          const int hrow = (CELL == GRU && row >= 2 * H) ? row + H : row;
          return dg[(size_t)hrow * B + b];
        });
        if (l > 0) tdot(acc2, Wih, K, k0, H, G * H, [&](int row) { return dg[(size_t)row * B + b]; });
#pragma unroll
        for (int u = 0; u < KB; ++u)
          if (k0 + u < H && lc.live) {
            const size_t kn = (size_t)(k0 + u) * n + lc.ii;
            dhc[kn] = dhc[kn] + acc[u];
            if (l > 0) ws.din[kn] = acc2[u];
          }
      }
      __syncthreads();
    }
  }
}

// Forward-mode derivative along the tangent `tv` (same layout as the parameters) through the recorded activations:
// out_dot [A][T][n].  With p = a gate's pre-activation: p_dot = V_ih x + v_bih + W_ih x_dot + V_hh h + v_bhh + W_hh h_dot.
// LIN: out_dot[q] = v_bias[q] + sum_k (v_kernel[q][k] a1[k] + kernel[q][k] [top[k] > 0] top_dot[k]).
template <int CELL, bool LIN = false, int NQ = 2>
__global__ void __launch_bounds__(SL *SW) k_stack_tangent(StackNet net, StackNet tv, StackWs ws, TrajDev tr,
                                                          float *__restrict__ out_dot,
                                                          const int32_t *__restrict__ skip) {
  if (skip != nullptr && *skip != 0) return;
  constexpr int G = gates<CELL>();
  const LaneCtx lc = lane_ctx(tr.n);
  const size_t n = tr.n, T = tr.T, B = T * n, plane = (T + 1) * n;
  const int H = net.H, H2 = net.H2, A = net.A, L = net.L;
  const float *__restrict__ W1 = net.p + net.off[L], *__restrict__ W2 = W1 + (size_t)H2 * H + H2;
  const float *__restrict__ V1 = tv.p + net.off[L], *__restrict__ vb1 = V1 + (size_t)H2 * H;
  const float *__restrict__ V2 = vb1 + H2, *__restrict__ vb2 = V2 + (size_t)A * H2;
  bool fresh = true;
  int cur = SET_TA;
  for (size_t t = 0; t < T; ++t) {
    const size_t b = t * n + lc.ii;
    const int nxt = cur == SET_TA ? SET_TB : SET_TA;
    for (int l = 0; l < L; ++l) {
      const int K = l == 0 ? net.D : H;
      const float *__restrict__ Wih = net.p + net.off[l], *__restrict__ Whh = Wih + (size_t)G * H * K;
      const float *__restrict__ Vih = tv.p + net.off[l], *__restrict__ Vhh = Vih + (size_t)G * H * K;
      const float *__restrict__ vbih = stack_bih<G>(tv, Vhh), *__restrict__ vbhh = stack_bhh<G>(tv, Vhh);
      const float *__restrict__ in = l == 0 ? tr.obs + t * n + lc.ii : rec_plane(ws, net, l - 1, RP_HOUT) + b;
      const size_t in_stride = l == 0 ? plane : B;
      const float *__restrict__ ind = l == 0 ? nullptr : slot(ws, net, nxt, 0, l - 1);
      const float *__restrict__ hprev = rec_plane(ws, net, l, RP_HPREV);
      const float *__restrict__ hd = slot(ws, net, cur, 0, l), *__restrict__ cd = slot(ws, net, cur, 1, l);
      float *__restrict__ hdn = slot(ws, net, nxt, 0, l), *__restrict__ cdn = slot(ws, net, nxt, 1, l);
      for (int j0 = UQ * lc.wave; j0 < H; j0 += UQ * SW) {
        float gidf[G * UQ], ghdf[G * UQ];
        int row[G * UQ];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int u = 0; u < UQ; ++u) {
            const int j = j0 + u < H ? j0 + u : H - 1;
            row[g * UQ + u] = g * H + j;
            gidf[g * UQ + u] = vbih[g * H + j];
            ghdf[g * UQ + u] = vbhh[g * H + j];
          }
        dot_rows(gidf, Vih, row, K, [&](int k) { return in[(size_t)k * in_stride]; });
        if (l > 0) dot_rows(gidf, Wih, row, K, [&](int k) { return ind[(size_t)k * n + lc.ii]; });
        dot_rows(ghdf, Vhh, row, H, [&](int k) { return hprev[(size_t)k * B + b]; });
        dot_rows(ghdf, Whh, row, H, [&](int k) { return fresh ? 0.0f : hd[(size_t)k * n + lc.ii]; });
        float gid[G][UQ], ghd[G][UQ];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int u = 0; u < UQ; ++u) {
            gid[g][u] = gidf[g * UQ + u];
            ghd[g][u] = ghdf[g * UQ + u];
          }
#pragma unroll
        for (int u = 0; u < UQ; ++u) {
          const int j = j0 + u;
          if (j >= H) break;
          const size_t jb = (size_t)j * B + b, jn = (size_t)j * n + lc.ii;
          float hnd;
          if (CELL == LSTM) {
            const float ig = rec_plane(ws, net, l, RP_G0)[jb], fg = rec_plane(ws, net, l, RP_G1)[jb];
            const float gg = rec_plane(ws, net, l, RP_G2)[jb], og = rec_plane(ws, net, l, RP_G3)[jb];
            const float cp = rec_plane(ws, net, l, RP_CPREV)[jb], tc = rec_plane(ws, net, l, RP_TC)[jb];
            const float i_d = ig * (1.0f - ig) * (gid[0][u] + ghd[0][u]);
            const float f_d = fg * (1.0f - fg) * (gid[1][u] + ghd[1][u]);
            const float g_d = (1.0f - gg * gg) * (gid[2][u] + ghd[2][u]);
            const float o_d = og * (1.0f - og) * (gid[G - 1][u] + ghd[G - 1][u]);
            const float cdp = fresh ? 0.0f : cd[jn];
            const float cn_d = f_d * cp + fg * cdp + i_d * gg + ig * g_d;
            const float tc_d = (1.0f - tc * tc) * cn_d;
            hnd = o_d * tc + og * tc_d;
            if (lc.live) cdn[jn] = cn_d;
          } else {
            const float r = rec_plane(ws, net, l, RP_G0)[jb], z = rec_plane(ws, net, l, RP_G1)[jb];
            const float nn = rec_plane(ws, net, l, RP_G2)[jb], ghn = rec_plane(ws, net, l, RP_G3)[jb];
            const float hp = hprev[jb];
            const float r_d = r * (1.0f - r) * (gid[0][u] + ghd[0][u]);
            const float z_d = z * (1.0f - z) * (gid[1][u] + ghd[1][u]);
            const float n_d = (1.0f - nn * nn) * (gid[2][u] + r_d * ghn + r * ghd[2][u]);
            const float hdp = fresh ? 0.0f : hd[jn];
            hnd = (hdp - n_d) * z + (hp - nn) * z_d + n_d;
          }
          if (lc.live) hdn[jn] = hnd;
        }
      }
      __syncthreads();
    }
    if (LIN) {
      if (lc.wave == 0) {
        const float *__restrict__ top = rec_plane(ws, net, L - 1, RP_HOUT);
        const float *__restrict__ topd = slot(ws, net, nxt, 0, L - 1);
        const float *__restrict__ vbk = V1 + (size_t)A * H;  // (W1 / V1: the Linear's kernel [A][H] and its tangent)
        if constexpr (NQ == 2) {
          const int qq[2] = {0, A > 1 ? 1 : 0};
          float od[2] = {vbk[qq[0]], vbk[qq[1]]};
          dot_rows(od, V1, qq, H, [&](int k) { return ws.a1[(size_t)k * B + b]; });
          dot_rows(od, W1, qq, H,
                   [&](int k) { return top[(size_t)k * B + b] > 0.0f ? topd[(size_t)k * n + lc.ii] : 0.0f; });
          if (lc.live)
            for (int q = 0; q < A; ++q) out_dot[(size_t)q * B + b] = od[q];
        } else {
          float od[NQ];
          head_passes(od, A, [&](int q) { return vbk[q]; }, [&](float (&acc)[UQ], const int (&qq)[UQ]) {
            dot_rows(acc, V1, qq, H, [&](int k) { return ws.a1[(size_t)k * B + b]; });
            dot_rows(acc, W1, qq, H,
                     [&](int k) { return top[(size_t)k * B + b] > 0.0f ? topd[(size_t)k * n + lc.ii] : 0.0f; });
          });
          if (lc.live) store_outputs(out_dot, B, b, od, A, true);
        }
      }
      fresh = tr.flag[b] != RL_SUCC_CONTINUE;
      cur = nxt;
      continue;
    }
    {
      const float *__restrict__ top = rec_plane(ws, net, L - 1, RP_HOUT);
      const float *__restrict__ topd = slot(ws, net, nxt, 0, L - 1);
      for (int j0 = UQ * lc.wave; j0 < H2; j0 += UQ * SW) {
        float acc[UQ];
        int jj[UQ];
#pragma unroll
        for (int u = 0; u < UQ; ++u) {
          jj[u] = j0 + u < H2 ? j0 + u : H2 - 1;
          acc[u] = vb1[jj[u]];
        }
        dot_rows(acc, V1, jj, H, [&](int k) { return ws.a1[(size_t)k * B + b]; });
        dot_rows(acc, W1, jj, H,
                 [&](int k) { return top[(size_t)k * B + b] > 0.0f ? topd[(size_t)k * n + lc.ii] : 0.0f; });
#pragma unroll
        for (int u = 0; u < UQ; ++u)
          if (j0 + u < H2 && lc.live)
            ws.u[(size_t)(j0 + u) * n + lc.ii] = ws.ur[(size_t)(j0 + u) * B + b] > 0.0f ? acc[u] : 0.0f;
      }
    }
    __syncthreads();
    if (lc.wave == 0) {
      if constexpr (NQ == 2) {
        const int qq[2] = {0, A > 1 ? 1 : 0};
        float od[2] = {vb2[qq[0]], vb2[qq[1]]};
        dot_rows(od, V2, qq, H2, [&](int j) { return ws.ur[(size_t)j * B + b]; });
        dot_rows(od, W2, qq, H2, [&](int j) { return ws.u[(size_t)j * n + lc.ii]; });
        if (lc.live)
          for (int q = 0; q < A; ++q) out_dot[(size_t)q * B + b] = od[q];
      } else {
        float od[NQ];
        head_passes(od, A, [&](int q) { return vb2[q]; }, [&](float (&acc)[UQ], const int (&qq)[UQ]) {
          dot_rows(acc, V2, qq, H2, [&](int j) { return ws.ur[(size_t)j * B + b]; });
          dot_rows(acc, W2, qq, H2, [&](int j) { return ws.u[(size_t)j * n + lc.ii]; });
        });
        if (lc.live) store_outputs(out_dot, B, b, od, A, true);
      }
    }
    fresh = tr.flag[b] != RL_SUCC_CONTINUE;
    cur = nxt;
  }
}

StackNet stack_net(const rl_mlp *m, const float *p) {
  StackNet s;
  s.p = p;
  s.z = m->has_bias ? nullptr : m->d_params + m->P;  // (the module's zeros also serve a tangent's absent bias entries)
  s.D = (int)m->in_dim;
  s.H = (int)m->gru_hidden;
  s.H2 = (int)m->hidden;
  s.A = (int)m->out_dim;
  s.L = (int)m->rnn_layers;
  for (uint32_t l = 0; l <= RL_RNN_MAX_LAYERS; ++l) s.off[l] = l <= m->rnn_layers ? (uint32_t)m->rnn_layer_offset(l) : 0;
  return s;
}

StackWs stack_ws(const rl_traj *t) {
  const SeqDev::Stack &k = t->seq.stack;
  StackWs w;
  w.st = k.st;
  w.u = k.u;
  w.din = k.din;
  w.dst = k.dst;
  w.rec = k.rec;
  w.a1 = k.a1;
  w.ur = k.ur;
  w.dg = k.dg;
  w.du = k.du;
  w.n = t->d.n;
  w.B = (uint64_t)t->d.T * t->d.n;
  return w;
}

inline uint32_t cdiv_k(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// the head's output-count class of a module (k_stack_forward / _step / _tangent are built at 2, 8 and 12): 2 for one or
// two outputs, 8 up to eight, 12 beyond (rl_rnn_chain_create_wide: at most RL_WIDE_MAX_OUT)
inline int out_class(const rl_mlp *m) {
  RL_REQUIRE(m->out_dim >= 1 && m->out_dim <= RL_WIDE_MAX_OUT, "recurrent chains: 1..12 outputs");
  return m->out_dim <= 2 ? 2 : (m->out_dim <= 8 ? 8 : 12);
}

}  // namespace

void stack_ensure(rl_traj *t, const rl_mlp *mod, bool training) {
  // (any recurrent chain: the modules of rl_mlp::lane_kernels always come here, and a recurrent DQN agent brings every
  // chain — a single-layer chain's flat order [W_ih, W_hh, b_ih, b_hh, head] IS the stacked order at L = 1, stack_net)
  RL_REQUIRE(rl_module_is_recurrent(mod->kind), "not a recurrent module");
  RL_REQUIRE(mod->in_dim == t->d.D, "module input width does not match the trajectory");
  SeqDev &q = t->seq;
  SeqDev::Stack &k = q.stack;
  const uint64_t n = t->d.n, T = t->d.T, B = T * n, L = mod->rnn_layers, H = mod->gru_hidden, H2 = mod->hidden;
  DevMem &mem = t->mem;
  seq_ensure_outputs(t);
  // a module of more than two outputs (rl_rnn_chain_create): one plane per output, grown where such a module first
  // meets the trajectory — the output planes, the rollout step's logits, and (training) lp0 / dz.  Grow-only: a
  // two-output module that follows uses the first two planes' worth of the same arrays at its own stride.
  const uint64_t A = mod->out_dim > 2 ? mod->out_dim : 2;
  mem.ensure(q.out, A * B);
  mem.ensure(q.succ, A * B);
  const bool lin = mod->linear_tail();  // no hidden units: no u / ur / du (a trajectory may serve both tails in turn)
  mem.ensure(k.st, 2 * N_SETS * L * H * n);
  if (!lin) mem.ensure(k.u, H2 * n);
  mem.ensure(k.z, A * n);
  if (!training) return;
  traj_ensure_action_planes(t, (uint32_t)A);
  mem.ensure(k.din, H * n);
  mem.ensure(k.dst, 2 * L * H * n);
  mem.ensure(k.rec, L * RPN * H * B);
  mem.ensure(k.a1, H * B);
  if (!lin) mem.ensure(k.ur, H2 * B);
  mem.ensure(k.dg, L * 4 * H * B);
  if (!lin) mem.ensure(k.du, H2 * B);
  // weight-gradient partials: at most 64 slab rows (the matrices are large: P doubles per row)
  uint64_t rows = t->nbA < 64 ? t->nbA : 64;
  uint64_t chunk = (B + rows - 1) / rows;
  chunk = ((chunk + 31) / 32) * 32;
  k.wg_chunk = (uint32_t)chunk;
  k.wg_rows = (uint32_t)((B + chunk - 1) / chunk);
  traj_ensure_slabs(t, k.wg_rows, mod->P, t->nbB);
  traj_ensure_pvec(t, mod->P);
}

void launch_stack_forward(rl_traj *traj, const rl_mlp *mod, float *d_out, float *d_succ, bool record,
                          const int32_t *d_skip) {
  ProfScope ps(traj->eng, RL_K_POLICY_FUSED);
  const StackNet net = stack_net(mod, mod->d_params);
  const StackWs ws = stack_ws(traj);
  const dim3 grid(cdiv_k(traj->d.n, SL)), blk(SL * SW);
#define FWD(CELL, REC, LIN, NQ)                                                                                       \
  hipLaunchKernelGGL((k_stack_forward<CELL, REC, LIN, NQ>), grid, blk, 0, traj->eng->stream, net, ws, traj->d, d_out, \
                     d_succ, d_skip)
#define FWD_TAIL(CELL, REC)                   \
  do {                                        \
    if (nq == 12) {                           \
      if (lin) FWD(CELL, REC, true, 12);      \
      else FWD(CELL, REC, false, 12);         \
    } else if (nq == 8) {                     \
      if (lin) FWD(CELL, REC, true, 8);       \
      else FWD(CELL, REC, false, 8);          \
    } else if (lin) FWD(CELL, REC, true, 2);  \
    else FWD(CELL, REC, false, 2);            \
  } while (0)
  // (`nq`: the output-count class of the head, stack_head)
  const bool lstm = mod->kind == RL_MODULE_LSTM_MLP, lin = mod->linear_tail();
  const int nq = out_class(mod);
  if (record) {
    if (lstm) FWD_TAIL(LSTM, true);
    else FWD_TAIL(GRU, true);
  } else {
    if (lstm) FWD_TAIL(LSTM, false);
    else FWD_TAIL(GRU, false);
  }
#undef FWD_TAIL
#undef FWD
  RL_HIP_CHECK(hipGetLastError());
}

void launch_stack_rollout(rl_env *env, const rl_mlp *policy, rl_traj *traj) {
  ProfScope ps(env->eng, RL_K_ROLLOUT);
  RL_REQUIRE(policy->out_dim >= 2 && policy->out_dim == env->A, "recurrent rollouts: one output per action of the env");
  const StackNet net = stack_net(policy, policy->d_params);
  const StackWs ws = stack_ws(traj);
  const dim3 grid(cdiv_k(traj->d.n, SL)), blk(SL * SW);
  float *z = traj->seq.stack.z;
  const bool lstm = policy->kind == RL_MODULE_LSTM_MLP, lin = policy->linear_tail();
  const int nq = out_class(policy);
  if (env->kind == RL_ENV_META_BANDIT && env->eng->kernel_variant != 1) {
    // meta-bandit lanes: all T steps in one launch (kernel variant 1 keeps the launch sequence per step, below).  Two to
    // twelve arms: k arms make k + 4 observation features (env_lanes.hpp, MetaOps).
    RL_REQUIRE(env->A >= 2 && env->A <= RL_WIDE_MAX_OUT && env->D == env->A + 4,
               "fused recurrent rollout on meta-bandit lanes: built for two to twelve arms (k + 4 features)");
#define ROLL(CELL, LIN, DD, AA)                                                                                          \
  hipLaunchKernelGGL((k_stack_rollout<CELL, MetaOps, DD, LIN, AA>), grid, blk, 0, env->eng->stream, net, ws, env->dev, \
                     env->st, traj->d, env->t_global)
#define ROLL_ARMS(CELL, LIN)                        \
  do {                                              \
    switch (env->A) {                               \
      case 2: ROLL(CELL, LIN, 6, 2); break;         \
      case 3: ROLL(CELL, LIN, 7, 3); break;         \
      case 4: ROLL(CELL, LIN, 8, 4); break;         \
      case 5: ROLL(CELL, LIN, 9, 5); break;         \
      case 6: ROLL(CELL, LIN, 10, 6); break;        \
      case 7: ROLL(CELL, LIN, 11, 7); break;        \
      case 8: ROLL(CELL, LIN, 12, 8); break;        \
      case 9: ROLL(CELL, LIN, 13, 9); break;        \
      case 10: ROLL(CELL, LIN, 14, 10); break;      \
      case 11: ROLL(CELL, LIN, 15, 11); break;      \
      default: ROLL(CELL, LIN, 16, 12); break;      \
    }                                               \
  } while (0)
    if (lstm) {
      if (lin) ROLL_ARMS(LSTM, true);
      else ROLL_ARMS(LSTM, false);
    } else {
      if (lin) ROLL_ARMS(GRU, true);
      else ROLL_ARMS(GRU, false);
    }
#undef ROLL_ARMS
#undef ROLL
    RL_HIP_CHECK(hipGetLastError());
    env->t_global += traj->d.T;
    return;
  }
  if (env->kind == RL_ENV_META_MDP && env->eng->kernel_variant != 1 &&
      meta_mdp_fused_shape(env->dev.mm.states, env->dev.mm.actions)) {
    // meta-MDP lanes at the shapes of META_MDP_FUSED_SHAPES (handle_spec.hpp): all T steps in one launch; every other
    // shape in range, and kernel variant 1, keep the launch sequence per step, below.  Trials have one length, so all
    // lanes of a run draw their tables at the same step: a serial section of wave 0, once per trial (MetaMdpOps::reset).
    const uint32_t S = env->dev.mm.states, A = env->dev.mm.actions;
    RL_REQUIRE(env->D == S + A + 4 && env->A == A, "fused recurrent rollout on meta-MDP lanes: S + A + 4 features");
#define ROLL(CELL, LIN, SS, AA)                                                                                       \
  hipLaunchKernelGGL((k_stack_rollout<CELL, MetaMdpOps, SS + AA + 4, LIN, AA>), grid, blk, 0, env->eng->stream, net, \
                     ws, env->dev, env->st, traj->d, env->t_global)
#define ROLL_SHAPES(CELL, LIN)                                  \
  do {                                                          \
    if (S == 2 && A == 2) ROLL(CELL, LIN, 2, 2);                \
    else if (S == 3 && A == 2) ROLL(CELL, LIN, 3, 2);           \
    else if (S == 4 && A == 3) ROLL(CELL, LIN, 4, 3);           \
    else if (S == 5 && A == 5) ROLL(CELL, LIN, 5, 5);           \
    else if (S == 8 && A == 4) ROLL(CELL, LIN, 8, 4);           \
    else ROLL(CELL, LIN, 4, 8);                                 \
  } while (0)
    if (lstm) {
      if (lin) ROLL_SHAPES(LSTM, true);
      else ROLL_SHAPES(LSTM, false);
    } else {
      if (lin) ROLL_SHAPES(GRU, true);
      else ROLL_SHAPES(GRU, false);
    }
#undef ROLL_SHAPES
#undef ROLL
    RL_HIP_CHECK(hipGetLastError());
    env->t_global += traj->d.T;
    return;
  }
  if (env->kind == RL_ENV_META_MDP && env->eng->kernel_variant != 1 && env->dev.mm.states > RL_META_MDP_MAX &&
      meta_mdp_wide_fused_shape(env->dev.mm.states, env->dev.mm.actions)) {
    // the lanes of rl_env_create_meta_mdp_wide at META_MDP_WIDE_FUSED_SHAPES (10 x 5, the reference's default): rows of
    // sixteen floats (MetaMdpWideOps), 19 features, five actions; 550 variates per lane in the trial's serial section
    RL_REQUIRE(env->dev.mm.states == 10 && env->A == 5 && env->D == 19,
               "fused recurrent rollout on wide meta-MDP lanes: built for 10 x 5");
#define ROLL(CELL, LIN)                                                                                               \
  hipLaunchKernelGGL((k_stack_rollout<CELL, MetaMdpWideOps, 19, LIN, 5>), grid, blk, 0, env->eng->stream, net, ws, \
                     env->dev, env->st, traj->d, env->t_global)
    if (lstm) {
      if (lin) ROLL(LSTM, true);
      else ROLL(LSTM, false);
    } else {
      if (lin) ROLL(GRU, true);
      else ROLL(GRU, false);
    }
#undef ROLL
    RL_HIP_CHECK(hipGetLastError());
    env->t_global += traj->d.T;
    return;
  }
  if (env->kind == RL_ENV_PARTITION && env->eng->kernel_variant != 1 && env->D == RL_PARTITION_MAX_OBS_DIM) {
    // PartitionGame lanes under a visible limit (24 features, the partition-game experiment's shape): all T steps in one
    // launch.  23 features (no or a latent limit) and kernel variant 1 keep the launch sequence per step, below.
    RL_REQUIRE(env->A == 2, "fused recurrent rollout on PartitionGame lanes: two actions");
#define ROLL(CELL, LIN)                                                                                             \
  hipLaunchKernelGGL((k_stack_rollout<CELL, PartitionOps, 24, LIN, 2>), grid, blk, 0, env->eng->stream, net, ws, \
                     env->dev, env->st, traj->d, env->t_global)
    if (lstm) {
      if (lin) ROLL(LSTM, true);
      else ROLL(LSTM, false);
    } else {
      if (lin) ROLL(GRU, true);
      else ROLL(GRU, false);
    }
#undef ROLL
    RL_HIP_CHECK(hipGetLastError());
    env->t_global += traj->d.T;
    return;
  }
  launch_rollout_stepwise(env, traj, z, [&](uint32_t step) {
    const int first = step == 0 ? 1 : 0, parity = (int)(step & 1);
    // (the step before has been recorded by now: its successor codes are in the trajectory)
    const uint8_t *flag_prev = traj->d.flag + (size_t)(step == 0 ? 0 : step - 1) * traj->d.n;
#define STEP(CELL, LIN, NQ)                                                                                         \
  hipLaunchKernelGGL((k_stack_step<CELL, LIN, NQ>), grid, blk, 0, env->eng->stream, net, ws, env->d_obs, flag_prev, \
                     first, parity, z)
#define STEP_OUT(CELL, LIN)              \
  do {                                   \
    if (nq == 12) STEP(CELL, LIN, 12);   \
    else if (nq == 8) STEP(CELL, LIN, 8); \
    else STEP(CELL, LIN, 2);             \
  } while (0)
    if (lstm) {
      if (lin) STEP_OUT(LSTM, true);
      else STEP_OUT(LSTM, false);
    } else {
      if (lin) STEP_OUT(GRU, true);
      else STEP_OUT(GRU, false);
    }
#undef STEP_OUT
#undef STEP
  });
}

namespace {
// k_stack_collect_dqn over more than two actions (rl_dqn_create_finite): index-env lanes alone.  The bandit of NA arms has
// 5 features and MemoryGame(NA, h) has NA + h [+ 1]: the (NA, D) pairs no env has are not built.
template <int CELL, bool LIN, int NA>
void collect_dqn_actions(uint32_t D, dim3 grid, dim3 blk, hipStream_t stream, const StackNet &net, const StackWs &ws,
                         const rl_env *env, const ReplayDev &rp, float *xobs, size_t xstride, uint32_t T, uint64_t p_int,
                         int always_explore, uint8_t *d_flags) {
  auto go = [&](auto d) {
    constexpr int DD = decltype(d)::value;
    if constexpr (DD == 5 || DD > NA)
      hipLaunchKernelGGL((k_stack_collect_dqn<CELL, IndexOps, DD, LIN, NA>), grid, blk, 0, stream, net, ws, env->dev,
                         env->st, rp, xobs, xstride, T, p_int, always_explore, d_flags, env->t_global);
    else
      throw RlError(RL_ERR_UNSUPPORTED, "recurrent DQN collection: no index env has this (actions, features) pair");
  };
  switch (D) {
    case 4: go(std::integral_constant<int, 4>{}); break;
    case 5: go(std::integral_constant<int, 5>{}); break;
    case 6: go(std::integral_constant<int, 6>{}); break;
    case 7: go(std::integral_constant<int, 7>{}); break;
    default: go(std::integral_constant<int, 8>{}); break;
  }
}
}  // namespace

void launch_stack_collect_dqn(rl_env *env, const rl_mlp *qnet, rl_traj *roll, const ReplayDev &rp, uint32_t T,
                              uint64_t p_int, int always_explore, uint8_t *d_flags) {
  ProfScope ps(env->eng, RL_K_ROLLOUT);
  RL_REQUIRE(rl_module_is_recurrent(qnet->kind) && qnet->out_dim == env->A && env->A >= 2 && env->A <= 8 &&
                 qnet->in_dim == env->D,
             "recurrent DQN collection: a recurrent chain of one output per action (2..8) over the env's features");
  RL_REQUIRE(roll->d.n == rp.N && roll->d.D == env->D, "recurrent DQN collection: workspace of another shape");
  const StackNet net = stack_net(qnet, qnet->d_params);
  const StackWs ws = stack_ws(roll);
  const dim3 grid(cdiv_k(rp.N, SL)), blk(SL * SW);
  const size_t xstride = (size_t)(roll->d.T + 1) * roll->d.n;
  const bool lstm = qnet->kind == RL_MODULE_LSTM_MLP, lin = qnet->linear_tail(), cartpole = env->kind == RL_ENV_CARTPOLE;
  const bool index_env = env->kind == RL_ENV_CHAIN || env->kind == RL_ENV_MEMORY || env->kind == RL_ENV_BANDIT;
  if (!(cartpole ? env->D == 4 || env->D == 5 : index_env && env->D >= 4 && env->D <= 8))
    throw RlError(RL_ERR_UNSUPPORTED, "recurrent DQN collection: CartPole lanes of 4 or 5 features, index-env lanes of 4..8");
  if (env->A > 2) {
    RL_REQUIRE(index_env, "recurrent DQN collection over more than two actions: index-env lanes");
#define COLLECT_NA(CELL, LIN, NA)                                                                                     \
  case NA:                                                                                                            \
    collect_dqn_actions<CELL, LIN, NA>(env->D, grid, blk, env->eng->stream, net, ws, env, rp, roll->d.obs, xstride, T, \
                                       p_int, always_explore, d_flags);                                              \
    break
#define COLLECT_ACTIONS(CELL, LIN) \
  do {                             \
    switch (env->A) {              \
      COLLECT_NA(CELL, LIN, 3);    \
      COLLECT_NA(CELL, LIN, 4);    \
      COLLECT_NA(CELL, LIN, 5);    \
      COLLECT_NA(CELL, LIN, 6);    \
      COLLECT_NA(CELL, LIN, 7);    \
      default:                     \
        COLLECT_NA(CELL, LIN, 8);  \
    }                              \
  } while (0)
    if (lstm) {
      if (lin) COLLECT_ACTIONS(LSTM, true);
      else COLLECT_ACTIONS(LSTM, false);
    } else {
      if (lin) COLLECT_ACTIONS(GRU, true);
      else COLLECT_ACTIONS(GRU, false);
    }
#undef COLLECT_ACTIONS
#undef COLLECT_NA
    RL_HIP_CHECK(hipGetLastError());
    return;
  }
#define COLLECT(CELL, LIN, ENV, DD)                                                                                      \
  hipLaunchKernelGGL((k_stack_collect_dqn<CELL, ENV, DD, LIN>), grid, blk, 0, env->eng->stream, net, ws, env->dev,      \
                     env->st, rp, roll->d.obs, xstride, T, p_int, always_explore, d_flags, env->t_global)
#define COLLECT_ENV(CELL, LIN)                            \
  do {                                                    \
    if (cartpole) {                                       \
      if (env->D == 5) COLLECT(CELL, LIN, CartPoleOps, 5); \
      else COLLECT(CELL, LIN, CartPoleOps, 4);            \
    } else {                                              \
      switch (env->D) {                                   \
        case 4: COLLECT(CELL, LIN, IndexOps, 4); break;   \
        case 5: COLLECT(CELL, LIN, IndexOps, 5); break;   \
        case 6: COLLECT(CELL, LIN, IndexOps, 6); break;   \
        case 7: COLLECT(CELL, LIN, IndexOps, 7); break;   \
        default: COLLECT(CELL, LIN, IndexOps, 8); break;  \
      }                                                   \
    }                                                     \
  } while (0)
  if (lstm) {
    if (lin) COLLECT_ENV(LSTM, true);
    else COLLECT_ENV(LSTM, false);
  } else {
    if (lin) COLLECT_ENV(GRU, true);
    else COLLECT_ENV(GRU, false);
  }
#undef COLLECT_ENV
#undef COLLECT
  RL_HIP_CHECK(hipGetLastError());
}

// dz [A][B] and the record of the last training forward -> vec[0..P): the reverse scan, then one weight-gradient
// launch per matrix (partials in slab rows), then the reduction
void launch_stack_backward(rl_traj *traj, const rl_mlp *mod, const int32_t *d_skip) {
  rl_engine *e = traj->eng;
  const StackNet net = stack_net(mod, mod->d_params);
  const StackWs ws = stack_ws(traj);
  const SeqDev::Stack &k = traj->seq.stack;
  const uint64_t n = traj->d.n, T = traj->d.T, B = T * n;
  const int H = net.H, H2 = net.H2, A = net.A, L = net.L, G = mod->kind == RL_MODULE_LSTM_MLP ? 4 : 3;
  const uint32_t P = (uint32_t)mod->P;
  {
    ProfScope ps(e, RL_K_POLICY_FUSED);
    const dim3 grid(cdiv_k(n, SL)), blk(SL * SW);
#define BWD(CELL, LIN) \
  hipLaunchKernelGGL((k_stack_backward<CELL, LIN>), grid, blk, 0, e->stream, net, ws, traj->d, traj->dz, d_skip)
    if (mod->kind == RL_MODULE_LSTM_MLP) {
      if (mod->linear_tail()) BWD(LSTM, true);
      else BWD(LSTM, false);
    } else {
      if (mod->linear_tail()) BWD(GRU, true);
      else BWD(GRU, false);
    }
#undef BWD
  }
  {
    ProfScope ps(e, RL_K_BACKWARD);
    auto wgrad = [&](const float *dY, int N, const float *X, size_t xs, int K, uint64_t offW, uint64_t offB) {
      launch_gen_wgrad_planes(traj, dY, (size_t)B, N, X, xs, K, (size_t)B, k.wg_chunk, k.wg_rows, P, (uint32_t)offW,
                              (uint32_t)offB, d_skip);
    };
    const size_t plane = (size_t)(T + 1) * n;
    for (int l = 0; l < L; ++l) {
      const int K = l == 0 ? net.D : H;
      const uint64_t oWih = net.off[l], oWhh = oWih + (uint64_t)G * H * K;
      // (layers without bias vectors: no bias columns in the flat vector)
      const uint64_t obih = mod->has_bias ? oWhh + (uint64_t)G * H * H : 0xFFFFFFFFull;
      const uint64_t obhh = mod->has_bias ? obih + (uint64_t)G * H : 0xFFFFFFFFull;
      const float *dg = k.dg + (size_t)l * 4 * H * B;
      const float *X = l == 0 ? traj->d.obs : k.rec + ((size_t)(l - 1) * RPN + RP_HOUT) * H * B;
      const float *hp = k.rec + ((size_t)l * RPN + RP_HPREV) * H * B;
      wgrad(dg, G * H, X, l == 0 ? plane : (size_t)B, K, oWih, obih);
      if (G == 4) {
        wgrad(dg, 4 * H, hp, (size_t)B, H, oWhh, obhh);
      } else {  // hidden side: rows [r; z] as on the input side, the n rows from the fourth plane
        wgrad(dg, 2 * H, hp, (size_t)B, H, oWhh, obhh);
        wgrad(dg + (size_t)3 * H * B, H, hp, (size_t)B, H, oWhh + (uint64_t)2 * H * H,
              mod->has_bias ? obhh + (uint64_t)2 * H : 0xFFFFFFFFull);
      }
    }
    if (mod->linear_tail()) {
      const uint64_t oKernel = net.off[L], oBias = oKernel + (uint64_t)A * H;
      wgrad(traj->dz, A, k.a1, (size_t)B, H, oKernel, oBias);
    } else {
      const uint64_t oW1 = net.off[L], ob1 = oW1 + (uint64_t)H2 * H, oW2 = ob1 + H2, ob2 = oW2 + (uint64_t)A * H2;
      wgrad(k.du, H2, k.a1, (size_t)B, H, oW1, ob1);
      wgrad(traj->dz, A, k.ur, (size_t)B, H2, oW2, ob2);
    }
    RL_HIP_CHECK(hipGetLastError());
  }
  launch_reduce(traj, P, true, false, k.wg_rows, 0);
}

void launch_stack_tangent(rl_traj *traj, const rl_mlp *mod, const float *d_tangent, const int32_t *d_skip) {
  ProfScope ps(traj->eng, RL_K_POLICY_FUSED);
  const StackNet net = stack_net(mod, mod->d_params), tv = stack_net(mod, d_tangent);
  const StackWs ws = stack_ws(traj);
  const dim3 grid(cdiv_k(traj->d.n, SL)), blk(SL * SW);
#define TAN(CELL, LIN, NQ)                                                                                  \
  hipLaunchKernelGGL((k_stack_tangent<CELL, LIN, NQ>), grid, blk, 0, traj->eng->stream, net, tv, ws, traj->d, \
                     traj->seq.out, d_skip)
#define TAN_OUT(CELL, LIN)                \
  do {                                    \
    if (nq == 12) TAN(CELL, LIN, 12);     \
    else if (nq == 8) TAN(CELL, LIN, 8);  \
    else TAN(CELL, LIN, 2);               \
  } while (0)
  const int nq = out_class(mod);
  if (mod->kind == RL_MODULE_LSTM_MLP) {
    if (mod->linear_tail()) TAN_OUT(LSTM, true);
    else TAN_OUT(LSTM, false);
  } else {
    if (mod->linear_tail()) TAN_OUT(GRU, true);
    else TAN_OUT(GRU, false);
  }
#undef TAN_OUT
#undef TAN
  RL_HIP_CHECK(hipGetLastError());
}
