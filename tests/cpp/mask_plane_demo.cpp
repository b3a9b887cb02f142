// mask_plane_demo.cpp — relearn_amd/csrc/mask_plane.hpp on the host: the layout of the kept relu' masks, its encode and
// its decode.  Exit status 0 and "ok" when every check holds; the first failure is printed and ends the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "relearn_amd/csrc/mask_plane.hpp"

static void fail(const char *what, long a, long b, long c) {
  std::printf("FAILED %s (%ld, %ld, %ld)\n", what, a, b, c);
  std::exit(1);
}

// a lane's two plane words from its 32 packed pairs, as the keeping pass builds them
static void encode_lane(const uint32_t (&pair)[mp::PAIRS], uint32_t (&w)[mp::WORDS]) {
  uint32_t grp[4];
  for (int t = 0; t < 4; ++t) grp[t] = mp::encode_group([&](int k) { return pair[8 * t + k]; });
  w[0] = mp::encode_word(grp[0], grp[1]);
  w[1] = mp::encode_word(grp[2], grp[3]);
}

int main() {
  const uint32_t value[4] = {0u, 0x3F80u, 0x3F800000u, mp::ONE_PAIR};
  long checks = 0;
  // the index arithmetic: q = 8 t + 4 s + i covers 0..31 once, and (word, position) is a bijection onto 2 x 16
  {
    bool seen[mp::PAIRS] = {false};
    for (int t = 0; t < 4; ++t)
      for (int s = 0; s < 2; ++s)
        for (int i = 0; i < 4; ++i) {
          const int q = mp::pair_index(t, s, i);
          if (q < 0 || q >= mp::PAIRS || seen[q]) fail("pair_index", t, s, i);
          seen[q] = true;
          if (mp::pair_word(q) != q / 16 || mp::pair_pos(q) != q % 16) fail("pair_word / pair_pos", q, 0, 0);
        }
    if (mp::tile_offset(3) != 1536u || mp::lane_offset(63) != 504u || mp::LANE_BYTES * 64u != mp::TILE_BYTES ||
        mp::WORDS * 4u != mp::LANE_BYTES)
      fail("offsets", 0, 0, 0);
    if (mp::plane_words(0) != 0 || mp::plane_words(1) != 128 || mp::plane_words(32) != 128 || mp::plane_words(33) != 256)
      fail("plane_words", 0, 0, 0);
  }
  // Every lane and every pair: one pair set to each of its four values on a background of all-zero and of all-one
  // pairs.  (The functions do not take the lane: a lane's words are its own 8 bytes, whatever the lane — the loop is the
  // statement of that, and checks the lane's byte range against its neighbours'.)
  uint32_t owner_bits[mp::WORDS] = {0u, 0u};  // which pair owns a bit: no two pairs may share one
  for (int lane = 0; lane < 64; ++lane) {
    if (mp::lane_offset(lane) + mp::LANE_BYTES > mp::TILE_BYTES) fail("lane range", lane, 0, 0);
    if (lane > 0 && mp::lane_offset(lane) != mp::lane_offset(lane - 1) + mp::LANE_BYTES) fail("lane stride", lane, 0, 0);
    for (int q = 0; q < mp::PAIRS; ++q)
      for (int background = 0; background < 2; ++background)
        for (int v = 0; v < 4; ++v) {
          uint32_t pair[mp::PAIRS], w[mp::WORDS];
          for (int k = 0; k < mp::PAIRS; ++k) pair[k] = background ? mp::ONE_PAIR : 0u;
          pair[q] = value[v];
          encode_lane(pair, w);
          for (int k = 0; k < mp::PAIRS; ++k) {
            if (mp::decode_pair(w, k) != pair[k]) fail("encode then decode", lane, q, k);
            ++checks;
          }
          // the bits pair q owns: position r of word q >> 4 for the low element, 16 + r for the high one
          if (background == 0) {
            const uint32_t r = (uint32_t)mp::pair_pos(q);
            const uint32_t want = ((v & 1) ? 1u << r : 0u) | ((v & 2) ? 1u << (16 + r) : 0u);
            if (w[mp::pair_word(q)] != want || w[1 - mp::pair_word(q)] != 0u) fail("bit position", lane, q, v);
          }
        }
  }
  for (int q = 0; q < mp::PAIRS; ++q) {
    const uint32_t mine = 0x00010001u << mp::pair_pos(q);
    if (owner_bits[mp::pair_word(q)] & mine) fail("two pairs share a bit", q, 0, 0);
    owner_bits[mp::pair_word(q)] |= mine;
  }
  if (owner_bits[0] != 0xFFFFFFFFu || owner_bits[1] != 0xFFFFFFFFu) fail("bits without an owner", 0, 0, 0);
  // the decode of each position gives exactly 0x3F80 / 0x3F800000 / their sum / 0
  for (int wd = 0; wd < mp::WORDS; ++wd)
    for (int r = 0; r < 16; ++r)
      for (int v = 0; v < 4; ++v) {
        uint32_t w[mp::WORDS] = {0u, 0u};
        w[wd] = ((v & 1) ? 1u << r : 0u) | ((v & 2) ? 1u << (16 + r) : 0u);
        const uint32_t got = mp::decode_pair(w, 16 * wd + r);
        if (got != value[v]) fail("decode of a position", wd, r, v);
        // ... and nothing in any other position
        for (int k = 0; k < mp::PAIRS; ++k)
          if (k != 16 * wd + r && mp::decode_pair(w, k) != 0u) fail("decode leaks", wd, r, k);
        // ... also with every other bit of the word set
        w[wd] |= ~(0x00010001u << r);
        w[1 - wd] = 0xFFFFFFFFu;
        if (mp::decode_pair(w, 16 * wd + r) != value[v]) fail("decode among set bits", wd, r, v);
        ++checks;
      }
  // all 2^16 patterns of one word's low halves (the high halves: the complement pattern, so both halves are driven)
  for (int wd = 0; wd < mp::WORDS; ++wd)
    for (uint32_t pat = 0; pat < 65536u; ++pat) {
      uint32_t pair[mp::PAIRS], w[mp::WORDS];
      for (int k = 0; k < mp::PAIRS; ++k) pair[k] = 0u;
      for (int r = 0; r < 16; ++r)
        pair[16 * wd + r] = ((pat >> r) & 1u ? 0x3F80u : 0u) | ((pat >> r) & 1u ? 0u : 0x3F800000u);
      encode_lane(pair, w);
      if (w[wd] != (pat | ((~pat & 0xFFFFu) << 16)) || w[1 - wd] != 0u) fail("encode of a pattern", wd, (long)pat, 0);
      for (int r = 0; r < 16; ++r)
        if (mp::decode_pair(w, 16 * wd + r) != pair[16 * wd + r]) fail("pattern round trip", wd, (long)pat, r);
      ++checks;
    }
  std::printf("ok %ld checks\n", checks);
  return 0;
}
