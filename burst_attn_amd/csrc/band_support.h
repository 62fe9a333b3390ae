// Band masks (sliding windows): the tile-range arithmetic of the band form
// of the kernels.
//
// Pair (q row i, kv row j) of a tile call is visible iff lo <= i - j <= hi.
// A kernel's workgroup owns 256 rows of one side and streams the other side
// in 64-row tiles: the forward and dq own q and stream kv, dK/dV own kv and
// stream q.  Everything below is written for "own row r, streamed row s,
// visible iff lo <= r - s <= hi"; the kv-owning kernels get that form by
// passing the band of s - r, ba_band_flip.
//
// Host-only, constexpr and free of HIP includes, so a plain C++17 compiler
// can build it (tests/test_band_support_cpu.py does).  The launchers and the
// kernels both take their arithmetic from here; ba_band_args is the one
// argument the band form of a kernel takes after its last parameter.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BA_BAND_FN __host__ __device__ constexpr
#else
#define BA_BAND_FN constexpr
#endif

constexpr int BA_BAND_TILE = 64;    // rows of a streamed tile
constexpr int BA_BAND_BLOCK = 256;  // rows a workgroup owns
constexpr int BA_BAND_WAVE = 32;    // rows a wave owns
// bounds are clamped to +-BA_BAND_MAX by the launchers, so that differences
// of row indices (< 2^31) and bounds stay inside 64 bits by a wide margin
// and the kernels' own int compares of (r - s) against a bound are exact
constexpr int64_t BA_BAND_MAX = (int64_t)1 << 30;

struct ba_band_args {
  int lo, hi;
};

BA_BAND_FN int ba_band_clamp(int64_t x) {
  return (int)(x < -BA_BAND_MAX ? -BA_BAND_MAX : x > BA_BAND_MAX ? BA_BAND_MAX : x);
}
// the band of (s - r) given that of (r - s): the kv-owning kernels' view
BA_BAND_FN ba_band_args ba_band_flip(ba_band_args b) { return {-b.hi, -b.lo}; }

BA_BAND_FN bool ba_band_visible(int r, int s, ba_band_args b) {
  return b.lo <= r - s && r - s <= b.hi;
}

// [lo, hi) streamed tiles that can hold a pair visible to block `blk` of the
// owning side (rows [256 blk, 256 blk + 255] below S_own).  Rows r0..r1 see
// the streamed rows [r0 - hi, r1 - lo], one interval because lo <= hi; cut to
// [0, S_str).  Empty is lo >= hi.  Exact: the first and the last tile of a
// non-empty range each hold a visible pair.
struct ba_tile_range {
  int lo, hi;
};
BA_BAND_FN ba_tile_range ba_band_block_tiles(int64_t blk, ba_band_args b,
                                             int64_t S_own, int64_t S_str) {
  const int64_t r0 = blk * BA_BAND_BLOCK;
  const int64_t r1 =
      r0 + BA_BAND_BLOCK - 1 < S_own - 1 ? r0 + BA_BAND_BLOCK - 1 : S_own - 1;
  int64_t s0 = r0 - b.hi, s1 = r1 - b.lo;
  if (s0 < 0) s0 = 0;
  if (s1 > S_str - 1) s1 = S_str - 1;
  if (r0 > r1 || s0 > s1 || b.lo > b.hi) return {0, 0};
  return {(int)(s0 / BA_BAND_TILE), (int)(s1 / BA_BAND_TILE) + 1};
}

// Wave level: the wave's 32 own rows start at r0, the streamed tile's 64
// rows at s0; r - s then spans [r0 - s0 - 63, r0 - s0 + 31].
// active: the tile can hold a visible pair of the wave's rows.
BA_BAND_FN bool ba_band_wave_active(int r0, int s0, ba_band_args b) {
  return r0 - s0 + (BA_BAND_WAVE - 1) >= b.lo &&
         r0 - s0 - (BA_BAND_TILE - 1) <= b.hi;
}
// inside: every pair of the wave's rows and the tile's rows is in the band
// (the tile then needs no band compare; whether it lies inside S_str is the
// kernel's own test).
BA_BAND_FN bool ba_band_wave_inside(int r0, int s0, ba_band_args b) {
  return r0 - s0 - (BA_BAND_TILE - 1) >= b.lo &&
         r0 - s0 + (BA_BAND_WAVE - 1) <= b.hi;
}

// Visible (256-row own block, 64-row streamed tile) pairs of a whole call:
// what a band leaves of the work, for the measurements' ideal ratio.
constexpr int64_t ba_band_tile_pairs(ba_band_args b, int64_t S_own,
                                     int64_t S_str) {
  int64_t n = 0;
  for (int64_t blk = 0; blk * BA_BAND_BLOCK < S_own; ++blk) {
    const ba_tile_range r = ba_band_block_tiles(blk, b, S_own, S_str);
    n += r.hi - r.lo;
  }
  return n;
}
