// kernels_seq_in.hip — the input side of the GRU chain's training passes at 6 to 24 observation features, as two
// block-parallel kernels on the bf16 matrix pipe (exact three-piece products, seq_pieces.hpp).
//
// W_ih x + b_ih, its tangent and its weight gradient have no dependence between steps.  At five features they sit inside
// the recurrent kernels of kernels_seq_train.hip as VALU loops with per-lane weight registers; at 24 features those loops
// do not fit the 256-register budget of two waves per SIMD, so here they run apart, over all (step, tile) blocks:
//   k_seq_in_proj    gi[g][unit][sample] = W_ih[g] x + b_ih[g] (g = r, z, n) into planes 0 .. 2 of every block of the
//                    record — k_gru_recur_fwd<0> reads its own 16 bytes per gate and M-tile and writes r, z, n over
//                    them — or, given a tangent vector, V_ih x + v_bih into planes 0 .. 2 of the static terms
//                    (k_seq_tangent_pre<0>).  No extra memory: the planes are the ones the consumer overwrites.
//   k_seq_in_wgrad   dW_ih[g] = sum over samples of delta_g x^T and db_ih[g], from d pre_r, d pre_z and the n gate's
//                    input-side d pre_n (dpre arrays 0 .. 2, the last written by k_gru_recur_bwd<0>).
// Both contract over ONE k-block of 32 padded input rows: rows 0 .. in_dim - 1 are the features, row in_dim is the
// constant one (its weight is the bias, its gradient column is db_ih), the rows above are zero and load nothing — one
// instantiation serves every in_dim of 6 .. 24.
#include "seq_pieces.hpp"

namespace {

// ---------------------------------------------------------------- input projection, all (step, tile) blocks in parallel
// Ownership and lane map are the recurrence's: eight waves, wave w owns the units [16 w, 16 w + 16) of all three gates;
// accumulator register i of lane l is (sample 16 mt + 4 (l >> 4) + i, unit 16 w + (l & 15)), so a lane's result of one
// gate and M-tile is one 16-byte store at rec_at.  B operand: this wave's rows of [W_ih | b_ih | 0] as 3 gates x 3
// pieces x 4 registers, built once per launch (no recurrent state competes for the registers here).  A operand: lane
// (n16, g4) holds rows 8 g4 .. 8 g4 + 7 of x~ for sample 16 mt + n16, read straight from the feature-major observation
// planes (per row, the sixteen lanes of a group read 64 contiguous bytes) and split into pieces in registers.
__global__ void __launch_bounds__(W16 * 64, 2)
    k_seq_in_proj(TrajDev tr, const float *__restrict__ vec, float *__restrict__ dst, int arrays, uint32_t tiles,
                  uint32_t blocks, const int32_t *__restrict__ skip) {
  if (skip != nullptr && *skip != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n16 = lane & 15, g4 = lane >> 4, j = 16 * wave + n16;
  const int D = (int)tr.D;
  const uint32_t N = tr.n, T = tr.T;
  const GruParams g = gru_params(vec, D, 1);  // (only W_ih and b_ih are read: in front of anything the outputs move)
  Frag wf[3][3];  // [gate][piece]: rows 8 g4 .. + 7 of [W_ih | b_ih | 0] for unit j
#pragma unroll
  for (int gte = 0; gte < 3; ++gte) {
    const int row = gte * GH + j;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = 8 * g4 + i;
      v[i] = k < D ? g.Wih[(size_t)row * D + k] : k == D ? g.bih[row] : 0.0f;
    }
    frags_of8(v, wf[gte]);
  }
  const size_t plane = (size_t)(T + 1) * N;
  for (uint32_t blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const uint32_t t = blk / tiles, lane0 = (blk % tiles) * TL;
    float *__restrict__ ob = dst + (size_t)blk * arrays * GH * TL;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      float x[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = 8 * g4 + i;
        x[i] = k < D ? tr.obs[(size_t)k * plane + (size_t)t * N + lane0 + (uint32_t)(16 * mt + n16)] : k == D ? 1.0f : 0.0f;
      }
      Frag fa[3];
      frags_of8(x, fa);
      const uint32_t row = rec_at(j, 16 * mt + 4 * g4);
#pragma unroll
      for (int gte = 0; gte < 3; ++gte)
        *reinterpret_cast<f32x4 *>(ob + (uint32_t)(gte * GH * TL) + row) = mfma_pieces(fa, wf[gte], (f32x4){0, 0, 0, 0});
    }
  }
}

// ---------------------------------------------------------------- input-side weight gradients
// out[row][col] = sum over samples of delta[row][sample] x~[col][sample]: 384 gate rows x 32 padded columns, twelve
// 32x32 tiles of v_mfma_f32_32x32x16_bf16 with the SAMPLE as contraction index (the manner of k_gru_wgrad_bf16: [row][16
// samples] piece images, wimg_at; a contiguous run of blocks per workgroup).  The delta arrays are [half][unit][16]
// records and the observation planes are feature-major, so sixteen consecutive samples of a gate row or of a feature are
// already a row of an operand image: nothing is transposed.
// Dealing: the two halves (M-tiles) of a block go to the two wave sets — waves 0-3 contract samples 0-15, waves 4-7
// samples 16-31 — and wave w accumulates the tiles 3 (w & 3) .. + 2, i.e. 96 gate rows x all 32 columns (48 accumulator
// registers); the two sets' sums are folded through LDS once, at the end.  A whole block (both halves: 72 KB of delta
// pieces, 6 KB of x~ pieces) is staged at a time, each thread splitting 24 delta values and two of x~; the next block's
// global loads are issued before the products and land under them, and two workgroups share a CU, so one stages while
// the other multiplies.
__global__ void __launch_bounds__(W16 * 64, 2)
    k_seq_in_wgrad(TrajDev tr, const float *__restrict__ dpre, float *__restrict__ slab, uint32_t P, uint32_t tiles,
                   uint32_t blocks, uint32_t blocks_per_chunk, const int32_t *__restrict__ skip) {
  __shared__ __attribute__((aligned(16))) unsigned short AP[2][3][3 * GH * 16];  // [half][piece]: delta rows (wimg_at)
  __shared__ __attribute__((aligned(16))) unsigned short BP[2][3][32 * 16];      // [half][piece]: rows of x~
  if (skip != nullptr && *skip != 0) return;
  const int q = threadIdx.x, lane = q & 63, wave = q >> 6;
  const int n = lane & 31, hf = lane >> 5;
  const int half = wave >> 2, tile0 = 3 * (wave & 3);
  const int D = (int)tr.D;
  const uint32_t N = tr.n, T = tr.T;
  const size_t plane = (size_t)(T + 1) * N;
  bt::f32x16 acc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) acc[i] = (bt::f32x16){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t b0 = blockIdx.x * blocks_per_chunk;
  const uint32_t b1 = b0 + blocks_per_chunk < blocks ? b0 + blocks_per_chunk : blocks;  // (none: a row of zeros)
  // staging: thread q takes samples 4 (q & 3) .. + 3 of unit q >> 2 in both halves of the three delta arrays, and sample
  // q & 31 of the rows q >> 5 and 16 + (q >> 5) of x~
  const int srow = q >> 2, scol = 4 * (q & 3);
  const int xs = q & 31, xr = q >> 5;
  f32x4 dl[2][3];
  float xv[2];
  auto fetch = [&](uint32_t blk) {
    const float *__restrict__ db = dpre + (size_t)blk * DPRE_ARR * GH * TL;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int g3 = 0; g3 < 3; ++g3)
        dl[h][g3] = *reinterpret_cast<const f32x4 *>(db + (uint32_t)(g3 * GH * TL) + rec_at(srow, 16 * h + scol));
    const uint32_t t = blk / tiles, lane0 = (blk % tiles) * TL;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k = xr + 16 * u;
      xv[u] = k < D ? tr.obs[(size_t)k * plane + (size_t)t * N + lane0 + (uint32_t)xs] : k == D ? 1.0f : 0.0f;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int g3 = 0; g3 < 3; ++g3) {
        uint32_t p[4][3];
#pragma unroll
        for (int i = 0; i < 4; ++i) bt::split3(dl[h][g3][i], p[i][0], p[i][1], p[i][2]);
#pragma unroll
        for (int c = 0; c < 3; ++c)
          *reinterpret_cast<uint64_t *>(&AP[h][c][wimg_at(g3 * GH + srow, scol)]) =
              (uint64_t)bt::pk(p[0][c], p[1][c]) | ((uint64_t)bt::pk(p[2][c], p[3][c]) << 32);
      }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      uint32_t p0, p1, p2;
      bt::split3(xv[u], p0, p1, p2);
      const int at = wimg_at(xr + 16 * u, xs & 15);
      BP[xs >> 4][0][at] = (unsigned short)p0;
      BP[xs >> 4][1][at] = (unsigned short)p1;
      BP[xs >> 4][2][at] = (unsigned short)p2;
    }
  };
  auto products = [&]() {  // this wave set's half: 16 samples, three tiles against the one 32-row x~ image
    Frag fb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) fb[c].x = *reinterpret_cast<const uint4 *>(&BP[half][c][wimg_at(n, 8 * hf)]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      Frag fa[3];
#pragma unroll
      for (int c = 0; c < 3; ++c)
        fa[c].x = *reinterpret_cast<const uint4 *>(&AP[half][c][wimg_at(32 * (tile0 + i) + n, 8 * hf)]);
#pragma unroll
      for (int pa = 2; pa >= 0; --pa)  // small terms first
#pragma unroll
        for (int pb = 2; pb >= 0; --pb)
          if (pa + pb < PIECE_ORDER) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[pa].v, fb[pb].v, acc[i], 0, 0, 0);
    }
  };
  if (b0 < b1) fetch(b0);
  for (uint32_t blk = b0; blk < b1; ++blk) {
    __syncthreads();  // the previous block's products have read the images
    stage();
    __syncthreads();
    if (blk + 1 < b1) fetch(blk + 1);  // lands under the products
    products();
  }
  // ---- fold the two wave sets, then this workgroup's row of partials: the W_ih and b_ih columns
  __syncthreads();
  float *fold = reinterpret_cast<float *>(&AP[0][0][0]);  // [wave & 3][tile][register][lane]: 48 KB of the 72
  if (half == 1)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) fold[(((wave & 3) * 3 + i) * 16 + r) * 64 + lane] = acc[i][r];
  __syncthreads();
  if (half == 1) return;
  float *__restrict__ out = slab + (size_t)blockIdx.x * P;
  const size_t obih = (size_t)3 * GH * D + (size_t)3 * GH * GH;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = acc[i][r] + fold[((wave * 3 + i) * 16 + r) * 64 + lane];
      const int row = 32 * (tile0 + i) + acc_row(r, hf);
      if (n < D) out[(size_t)row * D + n] = v;
      else if (n == D) out[obih + row] = v;  // the constant row's column: db_ih (the columns above it are not stored)
    }
}

}  // namespace

// ---------------------------------------------------------------- launchers
void launch_seq_in_proj(rl_traj *traj, const float *vec, float *dst, int arrays, const int32_t *d_skip) {
  RL_REQUIRE(traj->d.D >= 6 && traj->d.D <= 24 && traj->d.n % TL == 0, "input projection: 6 to 24 features, whole tiles");
  const uint32_t tiles = traj->d.n / TL, blocks = traj->d.T * tiles;
  hipLaunchKernelGGL(k_seq_in_proj, dim3(blocks < 2048 ? blocks : 2048), dim3(W16 * 64), 0, traj->eng->stream, traj->d, vec,
                     dst, arrays, tiles, blocks, d_skip);
}

void launch_seq_in_wgrad(rl_traj *traj, const rl_mlp *mod, const int32_t *d_skip) {
  RL_REQUIRE(seq_wide_tile_fits(traj, mod), "input-side weight gradients: the wide tile shape");
  const SeqDev &q = traj->seq;
  hipLaunchKernelGGL(k_seq_in_wgrad, dim3(q.chunks), dim3(W16 * 64), 0, traj->eng->stream, traj->d, q.dpre, q.wg_slab,
                     (uint32_t)mod->P, q.tiles, traj->d.T * q.tiles, q.blocks_per_chunk, d_skip);
}
