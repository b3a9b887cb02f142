// kernels_seq_fvp.hip — Fisher-vector products through time for the trust-region update over the recurrent chains:
// ONE pair of forward-mode tangent kernels (static terms over all blocks, then the recurrence per tile), templated on the
// cell; a cell (GruTangent / LstmTangent) supplies its gate count, its carried tangents, where its static terms are stored
// and its pointwise tangent.
#include "seq_common.hpp"

// =====================================================================================================
// Fisher-vector products through time (TRPO over the recurrent policy): J v by forward-mode differentiation.
// The tangent recurrence of a step needs W_hh h_dot (recurrent) and V_hh h (V = tangent parameters; h is known
// from the activation record, so this part is NOT recurrent).  It is split accordingly:
//   k_seq_tangent_pre : all (t, tile) blocks in parallel, tangent weights in registers:
//                       static terms V_hh h + v_bhh (+ V_ih x + v_bih), V1 relu(h') + v_b1, V2 u + v_b2
//   k_seq_tangent_rec : per tile, t ascending, the model's own W_hh / W1 slices in registers (as the forward):
//                       h_dot recurrence, u_dot, out_dot
// Reference: HessianVectorProduct::mat_vec_mul (src/torch/optimizers/conjugate_gradient.rs:312-338) — the double
// backward of the mean KL, which at theta_0 equals J^T (diag(p) - p p^T) J v / B.
// =====================================================================================================

// ---------------------------------------------------------------- what a cell supplies
//   NG            gate blocks of W_ih / W_hh;  NS: carried tangents per owned sample (st[0] is h_dot)
//   W1_LDS        k_seq_tangent_pre keeps the MLP layer's tangent operands in LDS instead of registers
//   store_static  the static part of every gate's pre-activation tangent -> planes 0..3 of the block's dpre arrays
//                 (gh = V_hh h + v_bhh, gi = V_ih x + v_bih); plane 4 is the MLP layer's, written by the kernel
//   step          the pointwise tangent of one (unit, sample): acc = W_hh h_dot per gate; returns h'_dot and updates the
//                 carried tangents, which restart from zero after an episode end
struct GruTangent {
  static constexpr int NG = 3, NS = 1;
  static constexpr bool W1_LDS = false;
  static __device__ __forceinline__ void store_static(float *__restrict__ sb, size_t o, const float (&gh)[NG],
                                                      const float (&gi)[NG]) {
    sb[(size_t)0 * GH * TL + o] = gh[0] + gi[0];  // static part of d(gh_r + gi_r)
    sb[(size_t)1 * GH * TL + o] = gh[1] + gi[1];
    sb[(size_t)2 * GH * TL + o] = gi[2];          // d gi_n
    sb[(size_t)3 * GH * TL + o] = gh[2];          // static part of d gh_n
  }
  static __device__ __forceinline__ float step(const float *__restrict__ ab, const float *__restrict__ sb, size_t o,
                                               const float (&acc)[NG], float (&st)[NS], bool ended) {
    const float rr = ab[(size_t)ACT_R * GH * TL + o], zz = ab[(size_t)ACT_Z * GH * TL + o];
    const float nn = ab[(size_t)ACT_N * GH * TL + o], ghn = ab[(size_t)ACT_GHN * GH * TL + o];
    const float hp = ab[(size_t)ACT_HPREV * GH * TL + o];
    const float rd = rr * (1.0f - rr) * (acc[0] + sb[(size_t)0 * GH * TL + o]);
    const float zd = zz * (1.0f - zz) * (acc[1] + sb[(size_t)1 * GH * TL + o]);
    const float ghd = acc[2] + sb[(size_t)3 * GH * TL + o];
    const float nd = (1.0f - nn * nn) * (sb[(size_t)2 * GH * TL + o] + rd * ghn + rr * ghd);
    const float v = (st[0] - nd) * zz + (hp - nn) * zd + nd;
    st[0] = ended ? 0.0f : v;
    return v;
  }
};

// p = pre-activation of a gate: p_dot = [V_hh h + v_bhh + V_ih x + v_bih] (static, stat[0..3]) + W_hh h_dot (recurrent);
// i_dot = i (1 - i) p_dot_i, f_dot, o_dot alike, g_dot = (1 - g^2) p_dot_g;
// c'_dot = f_dot c + f c_dot + i_dot g + i g_dot;  h'_dot = o_dot tanh(c') + o (1 - tanh(c')^2) c'_dot.
struct LstmTangent {
  static constexpr int NG = 4, NS = 2;  // st[1] is c_dot
  static constexpr bool W1_LDS = true;
  static __device__ __forceinline__ void store_static(float *__restrict__ sb, size_t o, const float (&gh)[NG],
                                                      const float (&gi)[NG]) {
#pragma unroll
    for (int gte = 0; gte < NG; ++gte) sb[(size_t)gte * GH * TL + o] = gh[gte] + gi[gte];
  }
  static __device__ __forceinline__ float step(const float *__restrict__ ab, const float *__restrict__ sb, size_t o,
                                               const float (&acc)[NG], float (&st)[NS], bool ended) {
    const float ig = ab[(size_t)LACT_I * GH * TL + o], fg = ab[(size_t)LACT_F * GH * TL + o];
    const float gg = ab[(size_t)LACT_G * GH * TL + o], og = ab[(size_t)LACT_O * GH * TL + o];
    const float cp = ab[(size_t)LACT_CPREV * GH * TL + o], tc = ab[(size_t)LACT_TC * GH * TL + o];
    const float id = ig * (1.0f - ig) * (acc[0] + sb[(size_t)0 * GH * TL + o]);
    const float fd = fg * (1.0f - fg) * (acc[1] + sb[(size_t)1 * GH * TL + o]);
    const float gd = (1.0f - gg * gg) * (acc[2] + sb[(size_t)2 * GH * TL + o]);
    const float od = og * (1.0f - og) * (acc[3] + sb[(size_t)3 * GH * TL + o]);
    const float cnd = fd * cp + fg * st[1] + id * gg + ig * gd;
    const float tcd = (1.0f - tc * tc) * cnd;
    const float v = od * tc + og * tcd;
    st[0] = ended ? 0.0f : v;
    st[1] = ended ? 0.0f : cnd;
    return v;
  }
};

template <int D, int A, class Cell>
__global__ void __launch_bounds__(256, 1) k_seq_tangent_pre(TrajDev tr, const float *__restrict__ tangent,
                                                            const float *__restrict__ act, float *__restrict__ stat,
                                                            float *__restrict__ out_stat, uint32_t tiles,
                                                            uint32_t blocks, uint32_t blocks_per_chunk,
                                                            const int32_t *__restrict__ skip) {
  constexpr int NG = Cell::NG;
  __shared__ float xS[TL][8];
  __shared__ float v2S[2][MH];
  // W1_LDS: the MLP layer's tangent operands, [k-step][thread] (read back by the thread that wrote them): the four gates'
  // 256 operand registers leave no room for these 64 next to the accumulators — the kernel spilt 45 registers with them
  __shared__ float w1S[Cell::W1_LDS ? GH / 2 : 1][Cell::W1_LDS ? 256 : 1];
  if (skip != nullptr && *skip != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 31, hf = lane >> 5, j = 32 * wave + n;
  const uint32_t N = tr.n, T = tr.T;
  const size_t plane = (size_t)(T + 1) * N;
  const GruParams v = seq_params(tangent, D, A, NG);
  // the forward's slicing (unit j = 32 * wave + (lane & 31), k parity = lane >> 5), applied to the tangent parameters
  float whh[NG][GH / 2], wih[NG][D], bih[NG], bhh[NG], w1[Cell::W1_LDS ? 1 : GH / 2];
#pragma unroll
  for (int gte = 0; gte < NG; ++gte) {
    const int row = gte * GH + j;
#pragma unroll
    for (int ks = 0; ks < GH / 2; ++ks) whh[gte][ks] = v.Whh[(size_t)row * GH + 2 * ks + hf];
#pragma unroll
    for (int d = 0; d < D; ++d) wih[gte][d] = v.Wih[(size_t)row * D + d];
    bih[gte] = v.bih[row];
    bhh[gte] = v.bhh[row];
  }
#pragma unroll
  for (int ks = 0; ks < GH / 2; ++ks) {
    const float w = v.W1[(size_t)j * GH + 2 * ks + hf];
    if constexpr (Cell::W1_LDS) w1S[ks][threadIdx.x] = w;
    else w1[ks] = w;
  }
  const float vb1 = v.b1[j];
  for (int q = threadIdx.x; q < A * MH; q += 256) v2S[q / MH][q % MH] = v.W2[q];
  const float vb2 = hf < A ? v.b2[hf] : 0.0f;
  const uint32_t b0 = blockIdx.x * blocks_per_chunk;
  const uint32_t b1 = b0 + blocks_per_chunk < blocks ? b0 + blocks_per_chunk : blocks;
  for (uint32_t blk = b0; blk < b1; ++blk) {
    const uint32_t t = blk / tiles, tile = blk % tiles, lane0 = tile * TL;
    const float *__restrict__ ab = act + (size_t)blk * SEQ_ARR * GH * TL;
    float *__restrict__ sb = stat + (size_t)blk * DPRE_ARR * GH * TL;
    __syncthreads();
    if (wave == 0 && lane < TL)
#pragma unroll
      for (int d = 0; d < D; ++d) xS[lane][d] = tr.obs[d * plane + (size_t)t * N + lane0 + lane];
    __syncthreads();
    f32x16 acc[NG];
#pragma unroll
    for (int gte = 0; gte < NG; ++gte)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[gte][r] = bhh[gte];
#pragma unroll
    for (int ks = 0; ks < GH / 2; ++ks) {
      const float a = ab[(size_t)ACT_HPREV * GH * TL + rec_at(2 * ks + hf, n)];
#pragma unroll
      for (int gte = 0; gte < NG; ++gte)
        acc[gte] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, whh[gte][ks], acc[gte], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = acc_row(r, hf);
      float gh[NG], gi[NG];
#pragma unroll
      for (int gte = 0; gte < NG; ++gte) {
        float q = bih[gte];
#pragma unroll
        for (int d = 0; d < D; ++d) q = __builtin_fmaf(xS[m][d], wih[gte][d], q);
        gi[gte] = q;
        gh[gte] = acc[gte][r];
      }
      Cell::store_static(sb, rec_at(j, m), gh, gi);
    }
    f32x16 acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc1[r] = vb1;
#pragma unroll
    for (int ks = 0; ks < GH / 2; ++ks) {
      float w;
      if constexpr (Cell::W1_LDS) w = w1S[ks][threadIdx.x];
      else w = w1[ks];
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ab[(size_t)ACT_A1 * GH * TL + rec_at(2 * ks + hf, n)], w, acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) sb[(size_t)4 * GH * TL + rec_at(j, acc_row(r, hf))] = acc1[r];
    if (wave == 0 && hf < A) {
      float z = vb2;
#pragma unroll 8
      for (int q = 0; q < MH; ++q) z = __builtin_fmaf(ab[(size_t)ACT_U * GH * TL + rec_at(q, n)], v2S[hf][q], z);
      out_stat[((size_t)hf * T + t) * N + lane0 + n] = z;
    }
  }
}

template <int A, class Cell>
__global__ void __launch_bounds__(256, 1) k_seq_tangent_rec(TrajDev tr, const float *__restrict__ params, int D,
                                                            const float *__restrict__ act,
                                                            const float *__restrict__ stat,
                                                            const float *__restrict__ out_stat,
                                                            float *__restrict__ out_dot,
                                                            const int32_t *__restrict__ skip) {
  constexpr int NG = Cell::NG, NS = Cell::NS;
  __shared__ float hdT[GH][TL + 1];
  __shared__ float a1dT[GH][TL + 1];
  __shared__ float udS[TL][MH + 1];
  __shared__ float w2S[2][MH];
  __shared__ int endS[TL];
  if (skip != nullptr && *skip != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 31, hf = lane >> 5, j = 32 * wave + n;
  const uint32_t N = tr.n, T = tr.T;
  const uint32_t tile = blockIdx.x, tiles = gridDim.x, lane0 = tile * TL;
  const GruParams g = seq_params(params, D, A, NG);
  float whh[NG][GH / 2], w1[GH / 2];
#pragma unroll
  for (int gte = 0; gte < NG; ++gte)
#pragma unroll
    for (int ks = 0; ks < GH / 2; ++ks) whh[gte][ks] = g.Whh[(size_t)(gte * GH + j) * GH + 2 * ks + hf];
#pragma unroll
  for (int ks = 0; ks < GH / 2; ++ks) w1[ks] = g.W1[(size_t)j * GH + 2 * ks + hf];
  for (int q = threadIdx.x; q < A * MH; q += 256) w2S[q / MH][q % MH] = g.W2[q];
  for (int q = threadIdx.x; q < GH * (TL + 1); q += 256) (&hdT[0][0])[q] = 0.0f;
  float st[16][NS];  // the carried tangents of the lane's 16 samples of unit j
#pragma unroll
  for (int r = 0; r < 16; ++r)
#pragma unroll
    for (int s = 0; s < NS; ++s) st[r][s] = 0.0f;
  __syncthreads();
  for (uint32_t t = 0; t < T; ++t) {
    const size_t blk = (size_t)t * tiles + tile;
    const float *__restrict__ ab = act + blk * SEQ_ARR * GH * TL;
    const float *__restrict__ sb = stat + blk * DPRE_ARR * GH * TL;
    if (wave == 0 && lane < TL) endS[lane] = tr.flag[(size_t)t * N + lane0 + lane] != RL_SUCC_CONTINUE;
    f32x16 acc[NG];
#pragma unroll
    for (int gte = 0; gte < NG; ++gte) acc[gte] = (f32x16){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < GH / 2; ++ks) {
      const float a = hdT[2 * ks + hf][n];
#pragma unroll
      for (int gte = 0; gte < NG; ++gte) acc[gte] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, whh[gte][ks], acc[gte], 0, 0, 0);
    }
    __syncthreads();  // every wave has read the old h_dot (and endS is visible)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = acc_row(r, hf);
      const size_t o = rec_at(j, m);
      const float a1 = ab[(size_t)ACT_A1 * GH * TL + o];
      float accr[NG];
#pragma unroll
      for (int gte = 0; gte < NG; ++gte) accr[gte] = acc[gte][r];
      const float v = Cell::step(ab, sb, o, accr, st[r], endS[m] != 0);  // (an ended episode's next step starts from zero)
      hdT[j][m] = st[r][0];
      a1dT[j][m] = a1 > 0.0f ? v : 0.0f;
    }
    __syncthreads();
    f32x16 acc1 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < GH / 2; ++ks)
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1dT[2 * ks + hf][n], w1[ks], acc1, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = acc_row(r, hf);
      const size_t o = rec_at(j, m);
      const float u = ab[(size_t)ACT_U * GH * TL + o];
      udS[m][j] = u > 0.0f ? acc1[r] + sb[(size_t)4 * GH * TL + o] : 0.0f;
    }
    __syncthreads();
    if (wave == 0 && hf < A) {
      float z = out_stat[((size_t)hf * T + t) * N + lane0 + n];
#pragma unroll 8
      for (int q = 0; q < MH; ++q) z = __builtin_fmaf(udS[n][q], w2S[hf][q], z);
      out_dot[((size_t)hf * T + t) * N + lane0 + n] = z;
    }
    __syncthreads();
  }
}

// dz <- (diag(p) - p p^T) out_dot / B with p = exp(log pi_0)  (the metric of the KL's Gauss-Newton form)
__global__ void __launch_bounds__(256) k_seq_fvp_dlogits(TrajDev tr, const float *__restrict__ out_dot,
                                                         const float *__restrict__ lp0, float *__restrict__ dz,
                                                         float inv_B, const int32_t *__restrict__ skip) {
  if (skip != nullptr && *skip != 0) return;
  const size_t B = (size_t)tr.T * tr.n;
  for (size_t b = (size_t)blockIdx.x * 256 + threadIdx.x; b < B; b += (size_t)gridDim.x * 256) {
    const float p0 = rl_expf(lp0[b]), p1 = rl_expf(lp0[B + b]);
    const float d0 = out_dot[b], d1 = out_dot[B + b];
    const float pdz = __builtin_fmaf(p1, d1, __builtin_fmaf(p0, d0, 0.0f));
    dz[b] = p0 * (d0 - pdz) * inv_B;
    dz[B + b] = p1 * (d1 - pdz) * inv_B;
  }
}

// ... over the A planes of a chain of more than two outputs: dz[q] = p_q (d_q - sum_r p_r d_r) / B, the inner sum an
// ascending fma chain from 0
template <int A>
__global__ void __launch_bounds__(256) k_seq_fvp_dlogits_n(TrajDev tr, const float *__restrict__ out_dot,
                                                           const float *__restrict__ lp0, float *__restrict__ dz,
                                                           float inv_B, const int32_t *__restrict__ skip) {
  if (skip != nullptr && *skip != 0) return;
  const size_t B = (size_t)tr.T * tr.n;
  for (size_t b = (size_t)blockIdx.x * 256 + threadIdx.x; b < B; b += (size_t)gridDim.x * 256) {
    float p[A], d[A];
    float pdz = 0.0f;
#pragma unroll
    for (int q = 0; q < A; ++q) {
      p[q] = rl_expf(lp0[(size_t)q * B + b]);
      d[q] = out_dot[(size_t)q * B + b];
      pdz = __builtin_fmaf(p[q], d[q], pdz);
    }
#pragma unroll
    for (int q = 0; q < A; ++q) dz[(size_t)q * B + b] = p[q] * (d[q] - pdz) * inv_B;
  }
}

// static terms over all blocks (-> seq.dpre, seq.succ), then the recurrence per tile (-> seq.out)
template <class Cell>
static void launch_seq_tangent(rl_traj *traj, const rl_mlp *mod, const float *d_tangent, const int32_t *d_skip) {
  rl_engine *e = traj->eng;
  const SeqDev &q = traj->seq;
  hipLaunchKernelGGL((k_seq_tangent_pre<5, 2, Cell>), dim3(q.chunks), dim3(256), 0, e->stream, traj->d, d_tangent, q.act,
                     q.dpre, q.succ, q.tiles, traj->d.T * q.tiles, q.blocks_per_chunk, d_skip);
  hipLaunchKernelGGL((k_seq_tangent_rec<2, Cell>), dim3(q.tiles), dim3(256), 0, e->stream, traj->d, mod->d_params, 5, q.act,
                     q.dpre, q.succ, q.out, d_skip);
}

void launch_gru_tangent(rl_traj *traj, const rl_mlp *mod, const float *d_tangent, uint64_t B_total,
                        const int32_t *d_skip) {
  rl_engine *e = traj->eng;
  const SeqDev &q = traj->seq;
  // (the tile kernels are two-action; a lane-kernel module may have up to eight outputs, rl_rnn_chain_create, or twelve,
  // rl_rnn_chain_create_wide)
  RL_REQUIRE(mod->out_dim == 2 || (mod->lane_kernels() && mod->out_dim > 2 && mod->out_dim <= RL_WIDE_MAX_OUT),
             "Fisher-vector products are for policies of two actions (lane-per-thread kernels: 2..12)");
  if (mod->lane_kernels()) launch_stack_tangent(traj, mod, d_tangent, d_skip);  // -> seq.out
  else {
    ProfScope ps(e, RL_K_POLICY_FUSED);
    if (mod->kind == RL_MODULE_LSTM_MLP) launch_seq_tangent<LstmTangent>(traj, mod, d_tangent, d_skip);
    else launch_seq_tangent<GruTangent>(traj, mod, d_tangent, d_skip);
  }
  {
    ProfScope ps(e, RL_K_POLICY_PASS);
#define FVN(AA)                                                                                                     \
  case AA:                                                                                                          \
    hipLaunchKernelGGL(k_seq_fvp_dlogits_n<AA>, dim3(traj->nbB), dim3(256), 0, e->stream, traj->d, q.out, traj->lp0, \
                       traj->dz, 1.0f / (float)B_total, d_skip);                                                    \
    break
    switch (mod->out_dim) {
      case 2:
        hipLaunchKernelGGL(k_seq_fvp_dlogits, dim3(traj->nbB), dim3(256), 0, e->stream, traj->d, q.out, traj->lp0,
                           traj->dz, 1.0f / (float)B_total, d_skip);
        break;
      FVN(3);
      FVN(4);
      FVN(5);
      FVN(6);
      FVN(7);
      FVN(8);
      FVN(9);  // 9..12: rl_rnn_chain_create_wide
      FVN(10);
      FVN(11);
      FVN(12);
      default: throw RlError(RL_ERR_UNSUPPORTED, "Fisher-vector products: 2..12 actions");
    }
#undef FVN
  }
}
