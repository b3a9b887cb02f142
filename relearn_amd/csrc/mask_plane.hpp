// mask_plane.hpp — the kept relu' masks of the fused 5-128-2 policy passes (kernels_mfma.hip): where a mask
// bit lives, how the gradient pass packs it and how the Fisher-vector pass turns it back into the packed bf16 pair the
// matrix pipe takes.  Host and device: the kernels use these functions, tests/cpp/mask_plane_demo.cpp compiles them
// with a host compiler.
//
// A wave's 32-sample tile has 32 x 128 masks; lane l holds the 64 of hidden unit (l & 31) of each of the four hidden
// tiles for the 16 samples of its half — as 32 packed bf16 PAIRS, the registers ga[t][s].u[i] of bt::mask_tile, each half
// 0x3F80 (1.0) or 0.  Pair q = 8 t + 4 s + i.  The plane keeps 8 bytes per (tile, lane), lane-linear: tile g begins at
// byte 512 g, lane l at 8 l inside it — one 8-byte load with a constant per-lane offset and the tile's offset as the
// scalar operand.  Pair q lives in word q >> 4 at position r = q & 15: the low element's bit at r, the high element's at
// 16 + r.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RL_MP_FN __host__ __device__ __forceinline__
#else
#define RL_MP_FN inline
#endif

namespace mp {

constexpr int PAIRS = 32;             // per (tile, lane)
constexpr int WORDS = 2;              // 32-bit words per (tile, lane)
constexpr uint32_t LANE_BYTES = 8u;   // per (tile, lane)
constexpr uint32_t TILE_BYTES = 512u; // 64 lanes
constexpr uint32_t ONE_PAIR = 0x3F803F80u;  // bf16 1.0 in both halves

RL_MP_FN constexpr int pair_index(int t, int s, int i) { return 8 * t + 4 * s + i; }
RL_MP_FN constexpr int pair_word(int q) { return q >> 4; }
RL_MP_FN constexpr int pair_pos(int q) { return q & 15; }
RL_MP_FN constexpr uint32_t tile_offset(uint32_t g) { return g * TILE_BYTES; }
RL_MP_FN constexpr uint32_t lane_offset(int lane) { return (uint32_t)lane * LANE_BYTES; }
// 32-bit words of a plane over `samples` samples (the ragged last tile is a whole tile)
RL_MP_FN constexpr uint64_t plane_words(uint64_t samples) { return (samples + 31) / 32 * (TILE_BYTES / 4); }

// ---- encode.  1.0 = 0x3F80 has bits 7..13 set, so pair k = 0..6 of a group of eight lends its bit 7 + k (and 23 + k)
// to the group word with ONE bit-select against a constant — no shift; the eighth pair has no bit 14 and is shifted up
// by one first.  A group word therefore holds pair k at bits 7 + k and 23 + k; two groups make a plane word with two
// shifts: nine + one vector instructions for eight pairs.
// pair(k): the packed pair 8 * group + k
template <typename F>
RL_MP_FN uint32_t encode_group(F pair) {
  uint32_t acc = pair(0) & (0x00010001u << 7);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 1; k < 7; ++k) {
    const uint32_t m = 0x00010001u << (7 + k);
    acc = (acc & ~m) | (pair(k) & m);
  }
  const uint32_t m = 0x00010001u << 14;
  return (acc & ~m) | ((pair(7) << 1) & m);
}
// groups 2 w and 2 w + 1 -> plane word w
RL_MP_FN uint32_t encode_word(uint32_t group_even, uint32_t group_odd) { return (group_even >> 7) | (group_odd << 1); }

// ---- decode.  (w & (0x00010001 << r)) * (0x3F80 >> r) for r < 8: the selected bits are r and 16 + r, 0x3F80 = 127 * 2^7
// is divisible by 2^r, so each set bit becomes exactly 0x3F80 in its half; both factors fit 24 bits (v_and_b32 with a
// literal, v_mul_u32_u24 with a literal).  Positions 8..15 decode the same way from w >> 8: one shift per eight pairs.
// (the compiler sees both factors' known bits and selects the 24-bit multiply itself)
RL_MP_FN uint32_t mul24(uint32_t a, uint32_t b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }
// the source of positions 8 h .. 8 h + 7 of word w
RL_MP_FN uint32_t decode_source(uint32_t w, int h) { return h == 0 ? w : w >> 8; }
// position r7 = r & 7 from its source
RL_MP_FN uint32_t decode_pos(uint32_t src, int r7) { return mul24(src & (0x00010001u << r7), 0x3F80u >> r7); }
// pair q of a lane's two words
RL_MP_FN uint32_t decode_pair(const uint32_t (&w)[WORDS], int q) {
  const int r = pair_pos(q);
  return decode_pos(decode_source(w[pair_word(q)], r >> 3), r & 7);
}

}  // namespace mp
