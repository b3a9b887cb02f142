// seq_recur_fwd.inc — the body of k_gru_recur_fwd<D> (REC = true) and k_gru_recur_eval<0> (REC = false), included into
// both (kernels_seq_train.hip).  In scope: D, REC, a1_plane; the arguments tr, params, A, act, skip.
  static_assert(REC || D == 0, "the record-less form reads gi from planes: input side elsewhere");
  constexpr int ARR = REC ? SEQ_ARR : DPRE_ARR;  // planes per block of `act`
  constexpr bool IN = D > 0;        // the input projection is this kernel's
  constexpr int DX = IN ? D : 1;
  __shared__ __attribute__((aligned(16))) unsigned short hP[3][TL * GH];  // h as pieces, [sample][unit] (img_at)
  __shared__ float xS[IN ? 2 : 1][IN ? TL : 1][9];  // (9: the four samples a wave reads at once are 4 rows apart — 144 bytes, not 128)
  __shared__ int endS[2][TL];
  __shared__ float wiS[IN ? 3 : 1][DX + 1][IN ? GH : 1];
  __shared__ uint4 wnS[GH / 32][3][W16][64];  // the n gate's W_hh fragments (96 KB): 48 registers the budget does not have
  if (skip != nullptr && *skip != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n16 = lane & 15, g4 = lane >> 4, j = 16 * wave + n16;
  const uint32_t N = tr.n, T = tr.T;
  const uint32_t tile = blockIdx.x, tiles = gridDim.x, lane0 = tile * TL;
  const GruParams g = gru_params(params, IN ? D : (int)tr.D, A);
  Frag wf[2][GH / 32][3];  // [gate r, z][k-block][piece]: W_hh[gate * GH + j][32 kb + 8 g4 + 0..7]
  float bhh[3];
#pragma unroll
  for (int gte = 0; gte < 3; ++gte) {
    const int row = gte * GH + j;
#pragma unroll
    for (int kb = 0; kb < GH / 32; ++kb) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = g.Whh[(size_t)row * GH + 32 * kb + 8 * g4 + i];
      if (gte < 2) {
        frags_of8(v, wf[gte][kb]);
      } else {
        Frag f[3];
        frags_of8(v, f);
#pragma unroll
        for (int q = 0; q < 3; ++q) wnS[kb][q][wave][lane] = f[q].x;
      }
    }
    bhh[gte] = g.bhh[row];
  }
  // the input projection's weights wait in LDS ([gate][feature | bias][unit]): 18 registers the products need more
  if constexpr (IN)
    for (int q = threadIdx.x; q < 3 * (D + 1) * GH; q += W16 * 64) {
      const int gte = q / ((D + 1) * GH), d = (q / GH) % (D + 1), u = q % GH;
      wiS[gte][d][u] = d < D ? g.Wih[(size_t)(gte * GH + u) * D + d] : g.bih[gte * GH + u];
    }
  for (int q = threadIdx.x; q < (int)(sizeof(hP) / 4); q += W16 * 64) reinterpret_cast<uint32_t *>(&hP[0][0])[q] = 0u;
  float hown[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) hown[r] = 0.0f;
  const bool io_lane = wave == 0 && lane < TL;
  const uint32_t i_lane = lane0 + (uint32_t)(lane & (TL - 1));
  const size_t plane = (size_t)(T + 1) * N;
  float xin[DX];
  int fin = 0;
  auto fetch = [&](uint32_t tt) {  // io lanes: observation and successor code of step tt, into registers
    if constexpr (IN)
#pragma unroll
      for (int d = 0; d < D; ++d) xin[d] = tr.obs[d * plane + (size_t)tt * N + i_lane];
    fin = tr.flag[(size_t)tt * N + i_lane];
  };
  auto publish = [&](int buf) {
    if constexpr (IN)
#pragma unroll
      for (int d = 0; d < D; ++d) xS[buf][lane][d] = xin[d];
    endS[buf][lane] = fin != RL_SUCC_CONTINUE;
  };
  if (io_lane) {
    fetch(0);
    publish(0);
  }
  // input side elsewhere: gi of (step, M-tile) in registers, loaded while the phase before it runs
  f32x4 gin[3][IN ? 1 : 2];
  auto fetch_gi = [&](uint32_t tt, int mt) {
    if constexpr (!IN) {
      const float *__restrict__ ab = act + ((size_t)tt * tiles + tile) * ARR * GH * TL;
      const uint32_t row = rec_at(j, 16 * mt + 4 * g4);
      gin[0][mt] = *reinterpret_cast<const f32x4 *>(ab + (uint32_t)(ACT_R * GH * TL) + row);
      gin[1][mt] = *reinterpret_cast<const f32x4 *>(ab + (uint32_t)(ACT_Z * GH * TL) + row);
      gin[2][mt] = *reinterpret_cast<const f32x4 *>(ab + (uint32_t)(ACT_N * GH * TL) + row);
    }
  };
  fetch_gi(0, 0);
  fetch_gi(0, 1);
  __syncthreads();
  // A step is two phases with a barrier after each, and in both the matrix pipe and the vector ALU work side by side:
  //   phase 1: products of M-tile 1 (step t)       | gate arithmetic of M-tile 0 (step t) -> rows 0-15 of h(t+1)
  //   phase 2: products of M-tile 0 (step t + 1)   | gate arithmetic of M-tile 1 (step t) -> rows 16-31 of h(t+1)
  // (the products of an M-tile need its 16 samples of ALL units, i.e. that M-tile's gate arithmetic of every wave, and
  // nothing of the other M-tile).  The barrier keeps the two waves of a SIMD in the same phase, so the overlap has to
  // come from INSIDE a wave: each phase is one basic block, and the scheduler is asked to place a few vector
  // instructions after every matrix instruction.  (One phase per step — both M-tiles' products, then both M-tiles'
  // gates with M-tile 1's products between M-tile 0's — left the first products and the last gates uncovered: VALU
  // busy 0.52 + matrix pipe 0.48 added up to the step time.)  Rows of the image are rewritten only after the barrier
  // that follows their last read, so one image serves.
  f32x4 acc[3][2];
  auto start = [&](int mt) {
#pragma unroll
    for (int gte = 0; gte < 3; ++gte) acc[gte][mt] = (f32x4){bhh[gte], bhh[gte], bhh[gte], bhh[gte]};
  };
  // operand reads run one k-block ahead of the products
  auto products = [&](int mt) {
    auto frags = [&](int kb, Frag (&a)[3]) {
#pragma unroll
      for (int p = 0; p < 3; ++p)
        a[p].x = *reinterpret_cast<const uint4 *>(&hP[p][img_at(16 * mt + n16, 32 * kb + 8 * g4)]);
    };
#pragma unroll
    for (int kb = 0; kb < GH / 32; ++kb) {
      Frag fa[3], wn[3];
      frags(kb, fa);
#pragma unroll
      for (int q = 0; q < 3; ++q) wn[q].x = wnS[kb][q][wave][lane];
#pragma unroll
      for (int gte = 0; gte < 2; ++gte) acc[gte][mt] = mfma_pieces(fa, wf[gte][kb], acc[gte][mt]);
      acc[2][mt] = mfma_pieces(fa, wn, acc[2][mt]);
    }
  };
  auto gates = [&](int mt, uint32_t t) {
    const int cur = (int)(t & 1);
    float *__restrict__ store = act + ((size_t)t * tiles + tile) * ARR * GH * TL;
    // (uniform block base + 32-bit lane offsets: the addresses stay out of the vector registers)
    const uint32_t row = rec_at(j, 16 * mt + 4 * g4);
    if constexpr (REC) {
      *reinterpret_cast<f32x4 *>(store + (uint32_t)(ACT_GHN * GH * TL) + row) = acc[2][mt];
      *reinterpret_cast<f32x4 *>(store + (uint32_t)(ACT_HPREV * GH * TL) + row) =
          (f32x4){hown[4 * mt], hown[4 * mt + 1], hown[4 * mt + 2], hown[4 * mt + 3]};
    }
    float wih[3][DX], bih[3];
    if constexpr (IN)
#pragma unroll
      for (int gte = 0; gte < 3; ++gte) {
#pragma unroll
        for (int d = 0; d < D; ++d) wih[gte][d] = wiS[gte][d][j];
        bih[gte] = wiS[gte][D][j];
      }
    f32x4 rv, zv, nv, av;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = acc16_row(mt, i, g4), r = 4 * mt + i;
      float gi[3];
#pragma unroll
      for (int gte = 0; gte < 3; ++gte) {
        if constexpr (IN) {
          float v = bih[gte];
#pragma unroll
          for (int d = 0; d < D; ++d) v = __builtin_fmaf(xS[cur][m][d], wih[gte][d], v);
          gi[gte] = v;
        } else {
          gi[gte] = gin[gte][mt][i];
        }
      }
      const float rr = sigmoid_sel(acc[0][mt][i] + gi[0]);
      const float zz = sigmoid_sel(acc[1][mt][i] + gi[1]);
      const float rn = acc[2][mt][i] * rr;
      const float nn = tanh_sel(gi[2] + rn);
      const float dn = hown[r] - nn;
      const float hz = dn * zz;
      const float hv = hz + nn;
      rv[i] = rr;
      zv[i] = zz;
      nv[i] = nn;
      av[i] = hv > 0.0f ? hv : 0.0f;
      // the state the next step starts from: zero after an episode end (SeqPacked restarts per episode)
      const float hn = endS[cur][m] != 0 ? 0.0f : hv;
      hown[r] = hn;
      uint32_t p0, p1, p2;
      bt::split3(hn, p0, p1, p2);
      hP[0][img_at(m, j)] = (unsigned short)p0;
      hP[1][img_at(m, j)] = (unsigned short)p1;
      hP[2][img_at(m, j)] = (unsigned short)p2;
    }
    if constexpr (REC) {
      *reinterpret_cast<f32x4 *>(store + (uint32_t)(ACT_R * GH * TL) + row) = rv;
      *reinterpret_cast<f32x4 *>(store + (uint32_t)(ACT_Z * GH * TL) + row) = zv;
      *reinterpret_cast<f32x4 *>(store + (uint32_t)(ACT_N * GH * TL) + row) = nv;
      *reinterpret_cast<f32x4 *>(store + (uint32_t)(ACT_A1 * GH * TL) + row) = av;
    } else {
      *reinterpret_cast<f32x4 *>(store + (uint32_t)a1_plane * (uint32_t)(GH * TL) + row) = av;
    }
    // (the last step reads its own block again: values nobody uses, no branch in the phase's block)
    fetch_gi(t + 1 < T ? t + 1 : t, mt);
  };
  // the order asked of the scheduler for a phase: one matrix instruction, a few vector ones (PHASE: the two phases share
  // a basic block, and groups of one sync id are matched against the whole block)
  auto interleave = [&](auto phase) {
    constexpr int PHASE = decltype(phase)::value;
#pragma unroll
    for (int k = 0; k < (GH / 32) * 3 * PIECE_PAIRS; ++k) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, PHASE);              // MFMA
      __builtin_amdgcn_sched_group_barrier(0x002, VALU_PER_MFMA, PHASE);  // VALU
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  start(0);
  products(0);  // (h = 0: the biases)
  for (uint32_t t = 0; t < T; ++t) {
    if (io_lane && t + 1 < T) fetch(t + 1);  // lands under the products
    __builtin_amdgcn_sched_barrier(0);
    start(1);
    gates(0, t);
    products(1);
    interleave(std::integral_constant<int, 0>{});
    __syncthreads();  // rows 0-15 of h(t+1) are complete; every wave has read rows 16-31 of h(t)
    // (the branch, always taken, gives phase 2 a basic block of its own: with both phases in one block the scheduler
    // honoured the requested order for one of them only)
    int taken;
    asm volatile("s_mov_b32 %0, 1" : "=s"(taken));
    if (taken != 0) {
      start(0);
      products(0);  // (after the last step: products nobody reads — a branch on t here would split the phase's block)
      gates(1, t);
      interleave(std::integral_constant<int, 1>{});
    }
    if (io_lane && t + 1 < T) publish((int)((t + 1) & 1));
    __syncthreads();  // rows 16-31 of h(t+1) and the inputs of step t + 1 are complete; rows 0-15 have been read
  }
