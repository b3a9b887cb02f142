// kernels_seq_head_n.hip — the head of an MLP-tail chain of MANY outputs, GRU(128) -> ReLU -> Linear(128, 128) -> ReLU ->
// Linear(128, A) with A of 3 to 12 (ChainConfig<GruConfig, MlpConfig> as a categorical policy: the RL² random-MDP and
// bandit experiments' default model), for the update passes of the wide tile shape (seq_wide_tile_fits, kernels.hpp).
// The input side (kernels_seq_in.hip) and the recurrence (kernels_seq_train.hip) do not depend on the head: they leave
// relu(h') in ACT_A1 of the record (an evaluation: in one workspace plane) and take d relu(h') from DPRE_DA1; the
// tangent recurrence of a linear tail (k_seq_tangent_rec<0, ..>, kernels_seq_fvp.hip) leaves a1_dot = [relu(h') > 0]
// h'_dot in plane DPRE_DU.  What the head adds between them is here, block-parallel over all (step, tile) blocks, in
// exact three-piece bf16 products (seq_pieces.hpp):
//   k_seq_head_n_forward<REC>  u = relu(W1 relu(h') + b1) (recorded when REC), out = W2 u + b2
//   k_seq_head_n_backward      d u_pre (on chip), d relu(h') into DPRE_DA1, and the head's weight gradients
//   k_seq_head_n_tangent       u_dot = [u > 0] (V1 relu(h') + vb1 + W1 a1_dot), out_dot = V2 u + vb2 + W2 u_dot
// The hidden layer has the ownership of k_seq_head_forward (eight waves per block, wave w owns the units [16 w, 16 w +
// 16), relu(h') as [sample][unit] piece images in LDS).  The OUTPUT layer is k_seq_lin_head's 16-row tile: out^T[a][m]
// = b2[a] + sum_k W2[a][k] u[k][m], rows 0 .. A - 1 live, the rows above zero and neither loaded nor stored; its B
// operand is u parked as [sample][unit] piece images.  A block has two M-tiles of 16 samples: waves 0 and 1 take one
// each, the other six have nothing to do in that phase (24 issues of 16 cycles against the hidden layer's 48 per wave:
// dealing the four k-blocks to more waves would add a cross-wave sum through LDS and a barrier for less than the barrier
// costs).  A is a launch argument; none of the kernels excludes an A inside 1 .. 12 — which modules come here is the
// predicate's decision (ModuleShape::wide_tile_shape).
// Flat order: [W_ih, W_hh, b_ih, b_hh, W1 [128][128], b1, W2 [A][128], b2 [A]] (seq_params, seq_common.hpp).
#include "seq_pieces.hpp"

namespace {

constexpr int HN_MAX_A = (int)RL_WIDE_MAX_OUT;
static_assert(HN_MAX_A <= 16, "the outputs are the live rows of ONE 16-row tile");
static_assert(GH == MH, "the piece images of relu(h') and u share one layout");

// the 16 x 8 values M[n16][32 kb + 8 g4 .. + 7] of a row-contiguous [A][128] matrix as the A operand of the 16-row
// tile (rows >= A: zeros)
__device__ __forceinline__ void rows_frag(const float *__restrict__ M, int A, int n16, int g4, int kb, Frag (&f)[3]) {
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = n16 < A ? M[(size_t)n16 * MH + 32 * kb + 8 * g4 + i] : 0.0f;
  frags_of8(v, f);
}

// the lane's four samples of M-tile mt of unit j -> their pieces in a [sample][unit] image
__device__ __forceinline__ void park4(unsigned short (*img)[TL * GH], const f32x4 &v, int mt, int g4, int j) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t p0, p1, p2;
    bt::split3(v[i], p0, p1, p2);
    const int m = acc16_row(mt, i, g4);
    img[0][img_at(m, j)] = (unsigned short)p0;
    img[1][img_at(m, j)] = (unsigned short)p1;
    img[2][img_at(m, j)] = (unsigned short)p2;
  }
}

// the operand fragments (sample 16 mt + n16, units 32 kb + 8 g4 .. + 7) of a [sample][unit] image
__device__ __forceinline__ void img_frag(unsigned short (*img)[TL * GH], int mt, int n16, int g4, int kb, Frag (&f)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) f[c].x = *reinterpret_cast<const uint4 *>(&img[c][img_at(16 * mt + n16, 32 * kb + 8 * g4)]);
}

// ---------------------------------------------------------------- head forward, with or without a record
// Per block: relu(h') (plane `plane` of the block's `arrays` planes of `act`) -> pieces in aK -> the hidden layer on
// the matrix pipe, this wave's 16 rows of W1 as register fragments -> u, stored to ACT_U when REC and parked as pieces
// in uK -> the output tile by waves 0 and 1, W2 split ONCE per launch into 4 k-blocks x 3 pieces (48 registers).
// Accumulator register i of the output tile in lane l is (output 4 (l >> 4) + i, sample 16 mt + (l & 15)): per
// output, sixteen lanes store 64 contiguous bytes of out[a][t][lane0 + ..].  The next block's relu(h') is fetched
// under this block's products.  REC = false is the same arithmetic statement for statement: the line search's
// candidate equal to theta_0 has ratios of exactly 1.
template <bool REC>
__global__ void __launch_bounds__(W16 * 64, 2)
    k_seq_head_n_forward(TrajDev tr, const float *__restrict__ params, int D, int NG, float *__restrict__ act, int arrays,
                         int plane, float *__restrict__ out, int A, uint32_t tiles, uint32_t blocks,
                         const int32_t *__restrict__ skip) {
  __shared__ __attribute__((aligned(16))) unsigned short aK[3][TL * GH];  // relu(h') as pieces (img_at)
  __shared__ __attribute__((aligned(16))) unsigned short uK[3][TL * MH];  // u as pieces (img_at)
  if (skip != nullptr && *skip != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n16 = lane & 15, g4 = lane >> 4, j = 16 * wave + n16;
  const uint32_t N = tr.n, T = tr.T;
  const GruParams g = seq_params(params, D, A, NG);
  Frag w1f[GH / 32][3];  // W1[j][32 kb + 8 g4 + 0..7]
#pragma unroll
  for (int kb = 0; kb < GH / 32; ++kb) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = g.W1[(size_t)j * GH + 32 * kb + 8 * g4 + i];
    frags_of8(v, w1f[kb]);
  }
  const float b1 = g.b1[j];
  const bool out_wave = wave < 2;  // the two M-tiles of the output layer
  Frag w2f[MH / 32][3];            // W2[n16][32 kb + 8 g4 + 0..7]
  f32x4 b2v = (f32x4){0, 0, 0, 0};
  if (out_wave) {
#pragma unroll
    for (int kb = 0; kb < MH / 32; ++kb) rows_frag(g.W2, A, n16, g4, kb, w2f[kb]);
#pragma unroll
    for (int i = 0; i < 4; ++i) b2v[i] = 4 * g4 + i < A ? g.b2[4 * g4 + i] : 0.0f;
  }
  const uint32_t lo = rec_at(j, 4 * g4);
  f32x4 a1n[2];
  auto fetch = [&](uint32_t blk) {
    const float *__restrict__ ab = act + ((size_t)blk * arrays + plane) * GH * TL;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) a1n[mt] = *reinterpret_cast<const f32x4 *>(ab + lo + REC_HALF * mt);
  };
  if (blockIdx.x < blocks) fetch(blockIdx.x);
  for (uint32_t blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const uint32_t t = blk / tiles, lane0 = (blk % tiles) * TL;
    __syncthreads();  // the previous block's readers of aK / uK are done
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) park4(aK, a1n[mt], mt, g4, j);
    if (blk + gridDim.x < blocks) fetch(blk + gridDim.x);  // the next block's operand lands under this block's products
    __syncthreads();
    f32x4 acc1[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) acc1[mt] = (f32x4){b1, b1, b1, b1};
#pragma unroll
    for (int kb = 0; kb < GH / 32; ++kb)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        Frag fa[3];
        img_frag(aK, mt, n16, g4, kb, fa);
        acc1[mt] = mfma_pieces(fa, w1f[kb], acc1[mt]);
      }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      f32x4 uv;
#pragma unroll
      for (int i = 0; i < 4; ++i) uv[i] = acc1[mt][i] > 0.0f ? acc1[mt][i] : 0.0f;
      park4(uK, uv, mt, g4, j);
      if constexpr (REC)
        *reinterpret_cast<f32x4 *>(act + ((size_t)blk * SEQ_ARR + ACT_U) * GH * TL + lo + REC_HALF * mt) = uv;
    }
    __syncthreads();
    if (out_wave) {  // M-tile `wave`: out^T[a][m] = b2[a] + sum_k W2[a][k] u[k][m]
      f32x4 acc = b2v;
#pragma unroll
      for (int kb = 0; kb < MH / 32; ++kb) {
        Frag fb[3];
        img_frag(uK, wave, n16, g4, kb, fb);
        acc = mfma_pieces(w2f[kb], fb, acc);
      }
      const size_t at = (size_t)t * N + lane0 + (uint32_t)(16 * wave + n16);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (4 * g4 + i < A) out[(size_t)(4 * g4 + i) * T * N + at] = acc[i];
    }
  }
}

// ---------------------------------------------------------------- head backward with the head's weight gradients
// k_gru_head_backward's structure (kernels_seq_train.hip): per block the three piece images uJ (d u_pre, [sample][unit]),
// uM (d u_pre, [unit][sample]) and aM (relu(h'), [unit][sample]); d relu(h') = [relu(h') > 0] d u_pre W1 into
// DPRE_DA1; dW1 with the sample as contraction index; db1 beside it.  What many outputs change:
//   dz[a][t][lane0 ..] of up to twelve outputs is staged into LDS by A x 32 threads (up to six waves).
//   d u_pre[m][j] = [u > 0] sum_a W2[a][j] dz[a][m] stays on the vector ALU: at most twelve terms per element, the unit's
//     W2 column in registers (a 32-row k-block of the matrix pipe would be more than half zeros).
//   dW2[a][j] += sum_m dz[a][m] u[j][m] on the matrix pipe, the block's 32 samples as the ONE k-block: A operand, lane
//     (n16, g4): row n16 of dz at the samples 4 g4 .. + 3, 16 + 4 g4 .. + 3 (from LDS); B operand: the same eight samples
//     of u of the lane's own unit — its two accumulator quadruples, already in registers.  Wave w keeps the columns
//     [16 w, 16 w + 16) of all rows in four accumulator registers for the whole walk.
//   db2[a] = sum_m dz[a][m]: wave 0 sums the A operand it holds.
// One row of f32 partials per workgroup: the head's columns of row blockIdx.x of `slab`.  The grid is ALWAYS
// RL_SEQ_HEAD_ROWS workgroups: one without a block writes its row of zeros, so the reduction's segment needs no memset.
__global__ void __launch_bounds__(W16 * 64, 2)
    k_seq_head_n_backward(TrajDev tr, const float *__restrict__ params, int D, int NG, const float *__restrict__ dz,
                          const float *__restrict__ act, float *__restrict__ dpre, float *__restrict__ slab, uint32_t P,
                          int A, uint32_t tiles, uint32_t blocks, const int32_t *__restrict__ skip) {
  __shared__ __attribute__((aligned(16))) unsigned short uJ[3][TL * GH];  // img_at
  __shared__ __attribute__((aligned(16))) unsigned short uM[3][MH * TL];  // timg_at
  __shared__ __attribute__((aligned(16))) unsigned short aM[3][GH * TL];  // timg_at
  __shared__ __attribute__((aligned(16))) float dzS[HN_MAX_A][TL];
  if (skip != nullptr && *skip != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n16 = lane & 15, g4 = lane >> 4, j = 16 * wave + n16;
  const uint32_t N = tr.n, T = tr.T;
  const size_t B = (size_t)T * N;
  const GruParams g = seq_params(params, D, A, NG);
  Frag w1f[MH / 32][3];  // B operand of d relu(h'): W1[32 kb + 8 g4 + 0..7][j] (rows: units of u; column: this lane's k)
#pragma unroll
  for (int kb = 0; kb < MH / 32; ++kb) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = g.W1[(size_t)(32 * kb + 8 * g4 + i) * GH + j];
    frags_of8(v, w1f[kb]);
  }
  float w2c[HN_MAX_A];
#pragma unroll
  for (int a = 0; a < HN_MAX_A; ++a) w2c[a] = a < A ? g.W2[a * MH + j] : 0.0f;
  f32x4 accw[GH / 16];  // dW1[16 wave + 4 g4 + i][16 nt + n16]
#pragma unroll
  for (int nt = 0; nt < GH / 16; ++nt) accw[nt] = (f32x4){0, 0, 0, 0};
  f32x4 accw2 = (f32x4){0, 0, 0, 0};  // dW2[4 g4 + i][j]
  float db1 = 0.0f, db2 = 0.0f;
  const uint32_t lo = rec_at(j, 4 * g4);
  const bool dz_thread = (int)threadIdx.x < A * TL;  // thread = (output tid >> 5, sample tid & 31)
  f32x4 a1n[2], un[2];
  float dzn = 0.0f;
  auto fetch = [&](uint32_t blk) {
    const float *__restrict__ ab = act + (size_t)blk * SEQ_ARR * GH * TL;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      a1n[mt] = *reinterpret_cast<const f32x4 *>(ab + (uint32_t)(ACT_A1 * GH * TL) + lo + REC_HALF * mt);
      un[mt] = *reinterpret_cast<const f32x4 *>(ab + (uint32_t)(ACT_U * GH * TL) + lo + REC_HALF * mt);
    }
    if (dz_thread) {
      const uint32_t t = blk / tiles, lane0 = (blk % tiles) * TL;
      dzn = dz[(size_t)(threadIdx.x >> 5) * B + (size_t)t * N + lane0 + (threadIdx.x & 31)];
    }
  };
  // this lane's eight samples of unit j (its two accumulator quadruples) -> chunk g4 of row j of each piece image
  auto park8 = [&](unsigned short (*img)[MH * TL], const f32x4 &v0, const f32x4 &v1) {
    uint32_t p[8][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bt::split3(v0[i], p[i][0], p[i][1], p[i][2]);
      bt::split3(v1[i], p[4 + i][0], p[4 + i][1], p[4 + i][2]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<uint4 *>(&img[c][timg_at(j, g4)]) =
          make_uint4(bt::pk(p[0][c], p[1][c]), bt::pk(p[2][c], p[3][c]), bt::pk(p[4][c], p[5][c]), bt::pk(p[6][c], p[7][c]));
  };
  if (blockIdx.x < blocks) fetch(blockIdx.x);
  for (uint32_t blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    float *__restrict__ db = dpre + (size_t)blk * DPRE_ARR * GH * TL;
    __syncthreads();  // the previous block's readers of the LDS images and of dzS are done
    if (dz_thread) dzS[threadIdx.x >> 5][threadIdx.x & 31] = dzn;
    f32x4 a1c[2], uc[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      a1c[mt] = a1n[mt];
      uc[mt] = un[mt];
    }
    park8(aM, a1c[0], a1c[1]);
    __syncthreads();  // dz of the block is visible
    if (blk + gridDim.x < blocks) fetch(blk + gridDim.x);  // the next block's operands land under this block's products
    {  // dW2 and db2: dz row n16 against this lane's u, both at the samples (4 g4 + i, 16 + 4 g4 + i)
      float za[8], ub[8];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const f32x4 z = n16 < A ? *reinterpret_cast<const f32x4 *>(&dzS[n16 < A ? n16 : 0][16 * mt + 4 * g4]) : (f32x4){0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          za[4 * mt + i] = z[i];
          ub[4 * mt + i] = uc[mt][i];
        }
      }
      Frag fa[3], fb[3];
      frags_of8(za, fa);
      frags_of8(ub, fb);
      accw2 = mfma_pieces(fa, fb, accw2);
      if (wave == 0)
#pragma unroll
        for (int i = 0; i < 8; ++i) db2 += za[i];
    }
    f32x4 duv[2];
    duv[0] = duv[1] = (f32x4){0, 0, 0, 0};
#pragma unroll
    for (int a = 0; a < HN_MAX_A; ++a)
      if (a < A) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          const f32x4 z = *reinterpret_cast<const f32x4 *>(&dzS[a][16 * mt + 4 * g4]);
#pragma unroll
          for (int i = 0; i < 4; ++i) duv[mt][i] = __builtin_fmaf(z[i], w2c[a], duv[mt][i]);
        }
      }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        duv[mt][i] = uc[mt][i] > 0.0f ? duv[mt][i] : 0.0f;
        db1 += duv[mt][i];
      }
      park4(uJ, duv[mt], mt, g4, j);
    }
    park8(uM, duv[0], duv[1]);
    __syncthreads();
    // d relu(h')[m][k = j] = sum over the units q of d u_pre[m][q] W1[q][k]
    f32x4 acc1[2];
    acc1[0] = acc1[1] = (f32x4){0, 0, 0, 0};
#pragma unroll
    for (int kb = 0; kb < MH / 32; ++kb)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        Frag fa[3];
        img_frag(uJ, mt, n16, g4, kb, fa);
        acc1[mt] = mfma_pieces(fa, w1f[kb], acc1[mt]);
      }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      f32x4 dav;
#pragma unroll
      for (int i = 0; i < 4; ++i) dav[i] = a1c[mt][i] > 0.0f ? acc1[mt][i] : 0.0f;
      *reinterpret_cast<f32x4 *>(db + (uint32_t)(DPRE_DA1 * GH * TL) + lo + REC_HALF * mt) = dav;
    }
    // dW1[row][col] += sum over the 32 samples of d u_pre[row][m] relu(h')[col][m]: A rows = this wave's 16 units
    {
      Frag fa[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) fa[c].x = *reinterpret_cast<const uint4 *>(&uM[c][timg_at(j, g4)]);
#pragma unroll
      for (int nt = 0; nt < GH / 16; ++nt) {
        Frag fb[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) fb[c].x = *reinterpret_cast<const uint4 *>(&aM[c][timg_at(16 * nt + n16, g4)]);
        accw[nt] = mfma_pieces(fa, fb, accw[nt]);
      }
    }
  }
  // ---- this workgroup's row of partials (head columns)
  const size_t oW1 = (size_t)NG * GH * D + (size_t)NG * GH * GH + 2 * NG * GH, ob1 = oW1 + (size_t)MH * GH, oW2 = ob1 + MH,
               ob2 = oW2 + (size_t)A * MH;
  float *__restrict__ out = slab + (size_t)blockIdx.x * P;
#pragma unroll
  for (int nt = 0; nt < GH / 16; ++nt)
#pragma unroll
    for (int i = 0; i < 4; ++i) out[oW1 + (size_t)(16 * wave + 4 * g4 + i) * GH + 16 * nt + n16] = accw[nt][i];
  // the four lane groups of a wave hold different samples of the same units
  db1 = db1 + __shfl_xor(db1, 16, 64);
  db1 = db1 + __shfl_xor(db1, 32, 64);
  if (g4 == 0) out[ob1 + j] = db1;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (4 * g4 + i < A) out[oW2 + (size_t)(4 * g4 + i) * MH + j] = accw2[i];
  if (wave == 0) {  // the four lane groups hold different samples of the same rows of dz
    db2 = db2 + __shfl_xor(db2, 16, 64);
    db2 = db2 + __shfl_xor(db2, 32, 64);
    if (g4 == 0 && n16 < A) out[ob2 + n16] = db2;
  }
}

// ---------------------------------------------------------------- the head's tangent, all blocks in parallel
// After the tangent recurrence (which carries no head work for these shapes) one launch forms, per block,
//   u_dot[m][j]   = [u > 0] (vb1[j] + sum_k V1[j][k] relu(h')[m][k] + sum_k W1[j][k] a1_dot[m][k])
//   out_dot[a][m] = vb2[a] + sum_k V2[a][k] u[m][k] + sum_k W2[a][k] u_dot[m][k]
// with V1, vb1, V2, vb2 the tangent vector's head slices: each line ONE contraction over K = 256, [relu(h') | a1_dot]
// against [V1 | W1] and [u | u_dot] against [V2 | W2].  relu(h') and u come from the record (ACT_A1, ACT_U), a1_dot from
// plane DPRE_DU of `stat`; u_dot exists only on chip.  Four [sample][unit] piece images in LDS (aK, dK, uK, eK: 96 KB);
// the first line has the hidden layer's ownership, wave w holding rows [16 w, 16 w + 16) of [V1 | W1] as 96 fragment
// registers; the second is the 16-row output tile on waves 0 and 1, its A operand [V2 | W2] split once per launch —
// wave w stages k-block w — into LDS (24 KB: 96 more registers would not fit beside the first line's).
__global__ void __launch_bounds__(W16 * 64, 2)
    k_seq_head_n_tangent(TrajDev tr, const float *__restrict__ params, const float *__restrict__ tangent, int D, int NG,
                         const float *__restrict__ act, const float *__restrict__ stat, float *__restrict__ out_dot, int A,
                         uint32_t tiles, uint32_t blocks, const int32_t *__restrict__ skip) {
  constexpr int KB = GH / 32;  // k-blocks of one half of a K = 256 contraction
  __shared__ __attribute__((aligned(16))) unsigned short aK[3][TL * GH];  // relu(h')
  __shared__ __attribute__((aligned(16))) unsigned short dK[3][TL * GH];  // a1_dot
  __shared__ __attribute__((aligned(16))) unsigned short uK[3][TL * MH];  // u
  __shared__ __attribute__((aligned(16))) unsigned short eK[3][TL * MH];  // u_dot
  __shared__ uint4 w2S[2 * KB][3][64];  // [V2 | W2] as A-operand fragments: [k-block][piece][lane]
  if (skip != nullptr && *skip != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n16 = lane & 15, g4 = lane >> 4, j = 16 * wave + n16;
  const uint32_t N = tr.n, T = tr.T;
  const GruParams g = seq_params(params, D, A, NG), v = seq_params(tangent, D, A, NG);
  Frag wf[2 * KB][3];  // [V1 | W1][j][32 kb + 8 g4 + 0..7]
#pragma unroll
  for (int kb = 0; kb < 2 * KB; ++kb) {
    const float *__restrict__ row = (kb < KB ? v.W1 : g.W1) + (size_t)j * GH + 32 * (kb % KB) + 8 * g4;
    float x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = row[i];
    frags_of8(x, wf[kb]);
  }
  const float vb1 = v.b1[j];
  {
    Frag f[3];
    rows_frag(wave < KB ? v.W2 : g.W2, A, n16, g4, wave % KB, f);
#pragma unroll
    for (int q = 0; q < 3; ++q) w2S[wave][q][lane] = f[q].x;
  }
  static_assert(W16 == 2 * KB, "one k-block of [V2 | W2] per wave");
  const bool out_wave = wave < 2;
  f32x4 vb2v = (f32x4){0, 0, 0, 0};
  if (out_wave)
#pragma unroll
    for (int i = 0; i < 4; ++i) vb2v[i] = 4 * g4 + i < A ? v.b2[4 * g4 + i] : 0.0f;
  const uint32_t lo = rec_at(j, 4 * g4);
  f32x4 a1n[2], adn[2], un[2];
  auto fetch = [&](uint32_t blk) {
    const float *__restrict__ ab = act + (size_t)blk * SEQ_ARR * GH * TL;
    const float *__restrict__ sb = stat + (size_t)blk * DPRE_ARR * GH * TL;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      a1n[mt] = *reinterpret_cast<const f32x4 *>(ab + (uint32_t)(ACT_A1 * GH * TL) + lo + REC_HALF * mt);
      un[mt] = *reinterpret_cast<const f32x4 *>(ab + (uint32_t)(ACT_U * GH * TL) + lo + REC_HALF * mt);
      adn[mt] = *reinterpret_cast<const f32x4 *>(sb + (uint32_t)(DPRE_DU * GH * TL) + lo + REC_HALF * mt);
    }
  };
  if (blockIdx.x < blocks) fetch(blockIdx.x);
  for (uint32_t blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const uint32_t t = blk / tiles, lane0 = (blk % tiles) * TL;
    __syncthreads();  // the previous block's readers of the images are done (first block: w2S is complete)
    f32x4 uc[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      park4(aK, a1n[mt], mt, g4, j);
      park4(dK, adn[mt], mt, g4, j);
      park4(uK, un[mt], mt, g4, j);
      uc[mt] = un[mt];
    }
    if (blk + gridDim.x < blocks) fetch(blk + gridDim.x);  // the next block's operands land under this block's products
    __syncthreads();
    f32x4 acc1[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) acc1[mt] = (f32x4){vb1, vb1, vb1, vb1};
#pragma unroll
    for (int kb = 0; kb < 2 * KB; ++kb)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        Frag fa[3];
        img_frag(kb < KB ? aK : dK, mt, n16, g4, kb % KB, fa);
        acc1[mt] = mfma_pieces(fa, wf[kb], acc1[mt]);
      }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      f32x4 ud;
#pragma unroll
      for (int i = 0; i < 4; ++i) ud[i] = uc[mt][i] > 0.0f ? acc1[mt][i] : 0.0f;
      park4(eK, ud, mt, g4, j);
    }
    __syncthreads();
    if (out_wave) {  // M-tile `wave`
      f32x4 acc = vb2v;
#pragma unroll
      for (int kb = 0; kb < 2 * KB; ++kb) {
        Frag fa[3], fb[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) fa[q].x = w2S[kb][q][lane];
        img_frag(kb < KB ? uK : eK, wave, n16, g4, kb % KB, fb);
        acc = mfma_pieces(fa, fb, acc);
      }
      const size_t at = (size_t)t * N + lane0 + (uint32_t)(16 * wave + n16);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (4 * g4 + i < A) out_dot[(size_t)(4 * g4 + i) * T * N + at] = acc[i];
    }
  }
}

void require_head_n(const rl_traj *traj, const rl_mlp *mod) {
  RL_REQUIRE(seq_wide_tile_fits(traj, mod) && !mod->linear_tail() && mod->out_dim >= 1 && mod->out_dim <= (uint32_t)HN_MAX_A,
             "many-output MLP head: the wide tile shape, an MLP tail of 1 to 12 outputs");
}

}  // namespace

// ---------------------------------------------------------------- launchers
void launch_seq_head_n_forward(rl_traj *traj, const rl_mlp *mod, float *d_out, float *d_act, int arrays, int plane,
                               bool record, const int32_t *d_skip) {
  require_head_n(traj, mod);
  RL_REQUIRE(!record || (arrays == SEQ_ARR && plane == ACT_A1), "many-output MLP head: a record is the training record");
  const uint32_t tiles = traj->d.n / TL, blocks = traj->d.T * tiles;
  const dim3 grid(blocks < 2048 ? blocks : 2048), wg(W16 * 64);
  const int D = (int)traj->d.D, NG = (int)rl_module_gates(mod->kind), A = (int)mod->out_dim;
  if (record)
    hipLaunchKernelGGL(k_seq_head_n_forward<true>, grid, wg, 0, traj->eng->stream, traj->d, mod->d_params, D, NG, d_act,
                       arrays, plane, d_out, A, tiles, blocks, d_skip);
  else
    hipLaunchKernelGGL(k_seq_head_n_forward<false>, grid, wg, 0, traj->eng->stream, traj->d, mod->d_params, D, NG, d_act,
                       arrays, plane, d_out, A, tiles, blocks, d_skip);
}

void launch_seq_head_n_backward(rl_traj *traj, const rl_mlp *mod, float *d_slab, const int32_t *d_skip) {
  require_head_n(traj, mod);
  const SeqDev &q = traj->seq;
  hipLaunchKernelGGL(k_seq_head_n_backward, dim3(RL_SEQ_HEAD_ROWS), dim3(W16 * 64), 0, traj->eng->stream, traj->d,
                     mod->d_params, (int)traj->d.D, (int)rl_module_gates(mod->kind), traj->dz, q.act, q.dpre, d_slab,
                     (uint32_t)mod->P, (int)mod->out_dim, q.tiles, traj->d.T * q.tiles, d_skip);
}

void launch_seq_head_n_tangent(rl_traj *traj, const rl_mlp *mod, const float *d_tangent, const int32_t *d_skip) {
  require_head_n(traj, mod);
  const SeqDev &q = traj->seq;
  const uint32_t blocks = traj->d.T * q.tiles;
  hipLaunchKernelGGL(k_seq_head_n_tangent, dim3(blocks < 512 ? blocks : 512), dim3(W16 * 64), 0, traj->eng->stream, traj->d,
                     mod->d_params, d_tangent, (int)traj->d.D, (int)rl_module_gates(mod->kind), q.act, q.dpre, q.out,
                     (int)mod->out_dim, q.tiles, blocks, d_skip);
}
