// kernels_seq_lin.hip — the head of a linear-tail chain, GRU(128) -> ReLU -> Linear(128, A) with A of 1 to 12 outputs
// (ChainConfig<GruConfig, LinearConfig>: the RL² experiments' policy and critic), for the training passes of the wide tile
// shape (seq_wide_tile_fits, kernels.hpp).  The input side (kernels_seq_in.hip) and the recurrence
// (kernels_seq_train.hip) do not depend on the head: they leave relu(h') in ACT_A1 of the record and take d relu(h')
// from DPRE_DA1.  What a linear tail adds between the two is here, block-parallel, in exact three-piece bf16 products
// (seq_pieces.hpp):
//   k_seq_lin_head           out^T[a][m] = init[a][m] + sum_k M[a][k] X[k][m] over every (step, tile) block — the forward
//                            (M = kernel, init = bias, X = relu(h')) and the two head terms of the tangent pass
//   k_seq_lin_head_backward  d relu(h') = [relu(h') > 0] kernel^T dz into DPRE_DA1, and the head's weight gradients
//                            dkernel = dz relu(h')^T, dbias = sum dz as one row of f32 partials per workgroup
// The flat order of such a module is [W_ih, W_hh, b_ih, b_hh, kernel [A][128], bias [A]]: the head starts at
// ModuleShape::rnn_layer_offset(1).  Neither kernel excludes an A inside 1 .. 12; which modules come here is the
// predicate's decision (ModuleShape::wide_tile_shape).
#include "seq_pieces.hpp"

namespace {

constexpr int LIN_MAX_A = (int)RL_WIDE_MAX_OUT;
constexpr int LIN_WAVES = 4;  // waves of a k_seq_lin_head workgroup: each walks blocks of its own
static_assert(LIN_MAX_A <= 16, "the outputs are the live rows of ONE 16-row tile");

// ---------------------------------------------------------------- out^T = init + M X, all (step, tile) blocks in parallel
// One 16-row tile of v_mfma_f32_16x16x32_bf16: rows 0 .. A - 1 are the outputs, the rows above are zero and are neither
// loaded nor stored.  A operand: M [A][128] row-contiguous — lane (n16, g4) holds M[n16][32 kb + 8 g4 .. + 7], split
// once per launch into 4 k-blocks x 3 pieces (48 registers).  B operand: the record plane X, [half][unit][16 samples] —
// lane (n16, g4) holds units 32 kb + 8 g4 .. + 7 of sample 16 mt + n16; for a fixed unit the sixteen lanes of a group
// read 64 contiguous bytes (k_seq_in_proj's access on the observation planes).  Accumulator register i of lane l is
// (output 4 (l >> 4) + i, sample 16 mt + (l & 15)): per output, sixteen lanes store 64 contiguous bytes of
// out[a][t][lane0 + ..].  One wave owns a whole block (2 M-tiles x 4 k-blocks x 6 piece pairs); no LDS, no barrier.
// `init`: the bias vector [A] (init_planes == 0) or planes [A][T][N] like `out`.
__global__ void __launch_bounds__(LIN_WAVES * 64)
    k_seq_lin_head(TrajDev tr, const float *__restrict__ M, const float *__restrict__ init, int init_planes,
                   const float *__restrict__ X, int arrays, int plane, float *__restrict__ out, int A, uint32_t tiles,
                   uint32_t blocks, const int32_t *__restrict__ skip) {
  if (skip != nullptr && *skip != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n16 = lane & 15, g4 = lane >> 4;
  const uint32_t N = tr.n, T = tr.T;
  const size_t B = (size_t)T * N;
  Frag mf[GH / 32][3];
#pragma unroll
  for (int kb = 0; kb < GH / 32; ++kb) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = n16 < A ? M[(size_t)n16 * GH + 32 * kb + 8 * g4 + i] : 0.0f;
    frags_of8(v, mf[kb]);
  }
  for (uint32_t blk = blockIdx.x * LIN_WAVES + wave; blk < blocks; blk += gridDim.x * LIN_WAVES) {
    const uint32_t t = blk / tiles, lane0 = (blk % tiles) * TL;
    const float *__restrict__ xb = X + ((size_t)blk * arrays + plane) * GH * TL;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const size_t at = (size_t)t * N + lane0 + (uint32_t)(16 * mt + n16);
      f32x4 acc;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int a = 4 * g4 + i;
        acc[i] = a < A ? (init_planes ? init[(size_t)a * B + at] : init[a]) : 0.0f;
      }
#pragma unroll
      for (int kb = 0; kb < GH / 32; ++kb) {
        float x[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = xb[rec_at(32 * kb + 8 * g4 + i, 16 * mt + n16)];
        Frag fb[3];
        frags_of8(x, fb);
        acc = mfma_pieces(mf[kb], fb, acc);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (4 * g4 + i < A) out[(size_t)(4 * g4 + i) * B + at] = acc[i];
    }
  }
}

// ---------------------------------------------------------------- head backward with the head's weight gradients
// A workgroup of eight waves walks blk = blockIdx.x, + gridDim.x, ..; lane (n16, g4) of wave w owns unit j = 16 w + n16
// and the samples 8 g4 .. 8 g4 + 7 of a block: 32 contiguous bytes of a [half][unit][16] record array, a wave's loads and
// stores 1 KB contiguous per half.
//   d relu(h')[j][m] = [relu(h')[j][m] > 0] sum_a kernel[a][j] dz[a][m] on the vector ALU: at most twelve terms per
//     element (a 32-row k-block of the matrix pipe would be more than half zeros); the unit's kernel column stays in
//     registers, dz[a][t][..] is read as 32-byte runs the sixteen lanes of a group share.
//   dkernel[a][j] += sum_m dz[a][m] relu(h')[j][m] on the matrix pipe with the SAMPLE as contraction index: the 32
//     samples of a block are one k-block.  A operand: lane (n16, g4) holds samples 8 g4 .. + 7 of dz row n16; B
//     operand: the same lane's eight samples of relu(h') of its unit — the values it has loaded for the mask.  Both are
//     32-byte runs straight from global memory: no transposition, no piece images in LDS.  Wave w keeps the columns
//     [16 w, 16 w + 16) of all rows in four accumulator registers for the whole walk.
//   dbias[a] = sum_m dz[a][m]: wave 0 sums the A operand it holds.
// One row of f32 partials per workgroup, the head's columns [ohead, P) of row blockIdx.x of `slab`.
__global__ void __launch_bounds__(W16 * 64)
    k_seq_lin_head_backward(TrajDev tr, const float *__restrict__ kernel, const float *__restrict__ dz,
                            const float *__restrict__ act, float *__restrict__ dpre, float *__restrict__ slab, uint32_t P,
                            uint32_t ohead, int A, uint32_t tiles, uint32_t blocks, const int32_t *__restrict__ skip) {
  if (skip != nullptr && *skip != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n16 = lane & 15, g4 = lane >> 4, j = 16 * wave + n16;
  const uint32_t N = tr.n, T = tr.T;
  const size_t B = (size_t)T * N;
  float kc[LIN_MAX_A];
#pragma unroll
  for (int a = 0; a < LIN_MAX_A; ++a) kc[a] = a < A ? kernel[(size_t)a * GH + j] : 0.0f;
  f32x4 accw = (f32x4){0, 0, 0, 0};
  float db = 0.0f;
  const uint32_t lo = rec_at(j, 8 * g4);
  for (uint32_t blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const uint32_t t = blk / tiles, lane0 = (blk % tiles) * TL;
    const float *__restrict__ a1p = act + ((size_t)blk * SEQ_ARR + ACT_A1) * GH * TL + lo;
    const float *__restrict__ dzb = dz + (size_t)t * N + lane0 + (uint32_t)(8 * g4);
    f32x4 a1v[2], zr[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      a1v[h] = *reinterpret_cast<const f32x4 *>(a1p + 4 * h);
      zr[h] = n16 < A ? *reinterpret_cast<const f32x4 *>(dzb + (size_t)n16 * B + 4 * h) : (f32x4){0, 0, 0, 0};
    }
    {
      float za[8], xa[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        za[i] = zr[i >> 2][i & 3];
        xa[i] = a1v[i >> 2][i & 3];
      }
      Frag fa[3], fb[3];
      frags_of8(za, fa);
      frags_of8(xa, fb);
      accw = mfma_pieces(fa, fb, accw);
      if (wave == 0)
#pragma unroll
        for (int i = 0; i < 8; ++i) db += za[i];
    }
    f32x4 d[2];
    d[0] = d[1] = (f32x4){0, 0, 0, 0};
#pragma unroll
    for (int a = 0; a < LIN_MAX_A; ++a)
      if (a < A) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x4 z = *reinterpret_cast<const f32x4 *>(dzb + (size_t)a * B + 4 * h);
#pragma unroll
          for (int i = 0; i < 4; ++i) d[h][i] = __builtin_fmaf(z[i], kc[a], d[h][i]);
        }
      }
    float *__restrict__ dp = dpre + ((size_t)blk * DPRE_ARR + DPRE_DA1) * GH * TL + lo;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4 dav;
#pragma unroll
      for (int i = 0; i < 4; ++i) dav[i] = a1v[h][i] > 0.0f ? d[h][i] : 0.0f;
      *reinterpret_cast<f32x4 *>(dp + 4 * h) = dav;
    }
  }
  // ---- this workgroup's row of partials: kernel [A][128], then bias [A]
  float *__restrict__ o = slab + (size_t)blockIdx.x * P + ohead;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (4 * g4 + i < A) o[(size_t)(4 * g4 + i) * GH + j] = accw[i];
  if (wave == 0) {  // the four lane groups hold different samples of the same rows
    db = db + __shfl_xor(db, 16, 64);
    db = db + __shfl_xor(db, 32, 64);
    if (g4 == 0 && n16 < A) o[(size_t)A * GH + n16] = db;
  }
}

}  // namespace

// ---------------------------------------------------------------- launchers
void launch_seq_lin_head(rl_traj *traj, const float *M, const float *init, bool init_planes, const float *X, int arrays,
                         int plane, float *d_out, int A, const int32_t *d_skip) {
  RL_REQUIRE(A >= 1 && A <= LIN_MAX_A && traj->d.n % TL == 0, "linear head: 1 to 12 outputs, whole tiles");
  const uint32_t tiles = traj->d.n / TL, blocks = traj->d.T * tiles, groups = (blocks + LIN_WAVES - 1) / LIN_WAVES;
  hipLaunchKernelGGL(k_seq_lin_head, dim3(groups < 2048 ? groups : 2048), dim3(LIN_WAVES * 64), 0, traj->eng->stream,
                     traj->d, M, init, init_planes ? 1 : 0, X, arrays, plane, d_out, A, tiles, blocks, d_skip);
}

void launch_seq_lin_head_forward(rl_traj *traj, const rl_mlp *mod, float *d_out, const float *d_act,
                                 const int32_t *d_skip) {
  const float *kernel = mod->d_params + mod->rnn_layer_offset(1);
  launch_seq_lin_head(traj, kernel, kernel + (size_t)mod->out_dim * GH, false, d_act, SEQ_ARR, ACT_A1, d_out,
                      (int)mod->out_dim, d_skip);
}

void launch_seq_lin_head_backward(rl_traj *traj, const rl_mlp *mod, float *d_slab, const int32_t *d_skip) {
  RL_REQUIRE(seq_wide_tile_fits(traj, mod) && mod->linear_tail(), "linear head backward: the wide tile shape, linear tail");
  const SeqDev &q = traj->seq;
  const uint32_t ohead = (uint32_t)mod->rnn_layer_offset(1);
  hipLaunchKernelGGL(k_seq_lin_head_backward, dim3(seq_lin_head_rows(traj)), dim3(W16 * 64), 0, traj->eng->stream, traj->d,
                     mod->d_params + ohead, traj->dz, q.act, q.dpre, d_slab, (uint32_t)mod->P, ohead, (int)mod->out_dim,
                     q.tiles, traj->d.T * q.tiles, d_skip);
}
