// seq_head_fwd.inc — the body of k_seq_head_forward<A> (REC = true) and k_seq_head_eval<A> (REC = false), included into
// both (kernels_seq_train.hip).  In scope: A, REC, arrays, plane; the arguments tr, params, D, NG, act, out, tiles,
// blocks, skip.
  __shared__ __attribute__((aligned(16))) unsigned short aK[3][TL * GH];  // relu(h') as pieces (img_at)
  __shared__ float vS[2][W16][TL];  // per output, wave and sample: the wave's 16 terms of W2 u
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
  float w2c[A];
#pragma unroll
  for (int a = 0; a < A; ++a) w2c[a] = g.W2[a * MH + j];
  const int ha = (int)threadIdx.x / TL, hm = (int)threadIdx.x % TL;  // threads < A TL: output, sample
  const float b2v = ha < A ? g.b2[ha] : 0.0f;
  const uint32_t lo = rec_at(j, 4 * g4);
  f32x4 a1n[2];
  auto fetch = [&](uint32_t blk) {
    if constexpr (REC) {
      const float *__restrict__ ab = act + (size_t)blk * SEQ_ARR * GH * TL;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
        a1n[mt] = *reinterpret_cast<const f32x4 *>(ab + (uint32_t)(ACT_A1 * GH * TL) + lo + REC_HALF * mt);
    } else {
      const float *__restrict__ ab = act + ((size_t)blk * arrays + plane) * GH * TL;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) a1n[mt] = *reinterpret_cast<const f32x4 *>(ab + lo + REC_HALF * mt);
    }
  };
  if (blockIdx.x < blocks) fetch(blockIdx.x);
  for (uint32_t blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const uint32_t t = blk / tiles, lane0 = (blk % tiles) * TL;
    [[maybe_unused]] float *__restrict__ ab = act + (size_t)blk * (REC ? SEQ_ARR : arrays) * GH * TL;  // (the record's block)
    __syncthreads();  // the previous block's readers of aK / vS are done
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint32_t p0, p1, p2;
        bt::split3(a1n[mt][i], p0, p1, p2);
        const int m = 16 * mt + 4 * g4 + i;
        aK[0][img_at(m, j)] = (unsigned short)p0;
        aK[1][img_at(m, j)] = (unsigned short)p1;
        aK[2][img_at(m, j)] = (unsigned short)p2;
      }
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
#pragma unroll
        for (int c = 0; c < 3; ++c)
          fa[c].x = *reinterpret_cast<const uint4 *>(&aK[c][img_at(16 * mt + n16, 32 * kb + 8 * g4)]);
        acc1[mt] = mfma_pieces(fa, w1f[kb], acc1[mt]);
      }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      f32x4 uv;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float u = acc1[mt][i] > 0.0f ? acc1[mt][i] : 0.0f;
        uv[i] = u;
#pragma unroll
        for (int a = 0; a < A; ++a) {
          const float part = sum16(u * w2c[a]);
          if (n16 == 0) vS[a][wave][acc16_row(mt, i, g4)] = part;
        }
      }
      if constexpr (REC) *reinterpret_cast<f32x4 *>(ab + (uint32_t)(ACT_U * GH * TL) + lo + REC_HALF * mt) = uv;
    }
    __syncthreads();
    if (ha < A) {
      float v = b2v;
#pragma unroll
      for (int w = 0; w < W16; ++w) v += vS[ha][w][hm];
      out[((size_t)ha * T + t) * N + lane0 + hm] = v;
    }
  }
