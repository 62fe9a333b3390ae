// Block masks (block-sparse attention): the tile lists of the block form of
// the kernels, their workspace layout, and the rule that builds them.
//
// A call carries a byte mask m[Bm][Hm][ceil(Sq / BS)][ceil(Sk / BS)], BS a
// power of two >= 64: pair (q row i, kv row j) is visible iff
// m[.][.][i / BS][j / BS] != 0, on top of the tensors' ranges and `causal`.
// A kernel's workgroup owns 256 rows of one side and streams the other in
// 64-row tiles (the forward and dq own q, dK/dV own kv).  The pre-pass turns
// the mask into one LIST of streamed tiles per (mask batch row, mask head, own
// block): the tiles, ascending, in which at least one of the workgroup's eight
// 32-row waves owns a set block.  An entry is
//     tile index | wave mask << 24
// bit w of the wave mask saying that wave w computes the tile.  Because
// BS >= 64 a tile lies in one block column and a wave's rows in one block
// row, so a set bit means that EVERY (row of the wave, row of the tile) pair
// is block-visible: the kernels need no per-element block test.  A bit is
// clear when the wave's rows start past S_own, and with `causal` when the
// tile lies wholly on the invisible side of the wave's rows; a tile past
// S_str is never listed.  With `causal` (Sq == Sk, so blocks are aligned on
// the diagonal) a set bit therefore leaves every row of the wave at least one
// visible key: the tile's first.
//
// Host-only, constexpr and free of HIP includes, like band_support.h: the
// pre-pass kernel, the launchers' bound check and a CPU test share it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BA_BLK_FN __host__ __device__ constexpr
#else
#define BA_BLK_FN constexpr
#endif

constexpr int BA_BLK_TILE = 64;    // rows of a streamed tile
constexpr int BA_BLK_BLOCK = 256;  // rows a workgroup owns
constexpr int BA_BLK_WAVE = 32;    // rows a wave owns
constexpr int BA_BLK_WAVES = BA_BLK_BLOCK / BA_BLK_WAVE;
constexpr int BA_BLK_MIN_LOG2 = 6;  // BS >= 64: a tile lies in one block
constexpr uint32_t BA_BLK_TILE_BITS = 24;
constexpr uint32_t BA_BLK_TILE_MASK = (1u << BA_BLK_TILE_BITS) - 1;
// tile indices must fit BA_BLK_TILE_BITS
constexpr int64_t BA_BLK_MAX_S = (int64_t)BA_BLK_TILE << BA_BLK_TILE_BITS;

BA_BLK_FN int64_t ba_blk_tiles(int64_t S) {
  return (S + BA_BLK_TILE - 1) / BA_BLK_TILE;
}
BA_BLK_FN int64_t ba_blk_blocks(int64_t S) {
  return (S + BA_BLK_BLOCK - 1) / BA_BLK_BLOCK;
}
BA_BLK_FN bool ba_blk_size_ok(int log2_bs) {
  return log2_bs >= BA_BLK_MIN_LOG2 && log2_bs <= 30;
}

// ---- workspace ------------------------------------------------------------
// 32-bit words; L = Bm * Hm lists per own block:
//   q_cnt   [L][blocks(Sq)]              entries of each q-owning list
//   q_list  [L][blocks(Sq)][tiles(Sk)]   kv tiles of the forward and dq
//   kv_cnt  [L][blocks(Sk)]
//   kv_list [L][blocks(Sk)][tiles(Sq)]   q tiles of dK/dV
// words = L * (blocks(Sq) * (1 + tiles(Sk)) + blocks(Sk) * (1 + tiles(Sq))).
// Every list has room for all streamed tiles, so this grows with Sq * Sk:
// 2 MiB per list set at Sq = Sk = 65536, 512 MiB at 2^20.
struct ba_blk_ws_layout {
  int64_t q_cnt, q_list, kv_cnt, kv_list, words;
};
BA_BLK_FN ba_blk_ws_layout ba_blk_ws(int64_t Bm, int64_t Hm, int64_t Sq,
                                     int64_t Sk) {
  const int64_t L = Bm * Hm;
  ba_blk_ws_layout w{};
  w.q_cnt = 0;
  w.q_list = w.q_cnt + L * ba_blk_blocks(Sq);
  w.kv_cnt = w.q_list + L * ba_blk_blocks(Sq) * ba_blk_tiles(Sk);
  w.kv_list = w.kv_cnt + L * ba_blk_blocks(Sk);
  w.words = w.kv_list + L * ba_blk_blocks(Sk) * ba_blk_tiles(Sq);
  return w;
}
BA_BLK_FN int64_t ba_blk_ws_bytes(int64_t Bm, int64_t Hm, int64_t Sq,
                                  int64_t Sk) {
  return ba_blk_ws(Bm, Hm, Sq, Sk).words * 4;
}

// ---- the list rule ----------------------------------------------------------
// One (mask batch row, mask head) plane of the mask as the owning side sees
// it: element (own block row, streamed block column) at m[r * s_own +
// c * s_str].  The q-owning kernels pass the mask's own strides, the
// kv-owning ones swap them: the bitmap is its own transpose source.
struct ba_blk_plane {
  const uint8_t* m;
  int64_t s_own, s_str;
  int log2_bs;
};

// Wave mask of (own block `blk`, streamed tile `t`).  own_is_q says which
// side of the diagonal `causal` hides: a q-owning wave at rows r0.. sees
// tile t iff 64 t <= r0 + 31, a kv-owning one iff 64 t + 63 >= r0.
BA_BLK_FN uint32_t ba_blk_wave_mask(const ba_blk_plane& p, int64_t blk,
                                    int64_t t, int64_t S_own, int64_t S_str,
                                    bool causal, bool own_is_q) {
  const int64_t s0 = t * BA_BLK_TILE;
  if (s0 >= S_str) return 0;
  const int64_t col = s0 >> p.log2_bs;
  uint32_t wm = 0;
  for (int w = 0; w < BA_BLK_WAVES; ++w) {
    const int64_t r0 = blk * BA_BLK_BLOCK + w * BA_BLK_WAVE;
    if (r0 >= S_own) break;
    if (causal && (own_is_q ? s0 > r0 + BA_BLK_WAVE - 1
                            : s0 + BA_BLK_TILE - 1 < r0))
      continue;
    if (p.m[(r0 >> p.log2_bs) * p.s_own + col * p.s_str]) wm |= 1u << w;
  }
  return wm;
}

BA_BLK_FN uint32_t ba_blk_entry(int64_t t, uint32_t wave_mask) {
  return (uint32_t)t | wave_mask << BA_BLK_TILE_BITS;
}

// The list of own block `blk`, as the pre-pass writes it: the entries go to
// out[0 .. n), n is returned.  The reference the CPU test compares with.
constexpr int64_t ba_blk_build_list(const ba_blk_plane& p, int64_t blk,
                                    int64_t S_own, int64_t S_str, bool causal,
                                    bool own_is_q, uint32_t* out) {
  int64_t n = 0;
  for (int64_t t = 0; t < ba_blk_tiles(S_str); ++t) {
    const uint32_t wm =
        ba_blk_wave_mask(p, blk, t, S_own, S_str, causal, own_is_q);
    if (wm) out[n++] = ba_blk_entry(t, wm);
  }
  return n;
}
