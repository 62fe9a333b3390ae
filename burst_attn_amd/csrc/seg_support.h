// Segment ids (packed sequences): which knob selections support them, and
// the layout of the workspace their pre-pass writes.
//
// Host-only and free of HIP includes, so a plain C++17 compiler can build
// it (tests/test_seg_support_cpu.py does).  The launchers and the pre-pass
// both take their arithmetic from here.
#pragma once
#include <stdint.h>

#include "bwd_plans.h"
#include "fwd_variants.h"

// nullptr knob = supported; else the env name and value that rule ids out
struct ba_seg_verdict {
  const char* knob;
  int value;
};

// Forward: the production variant only.  A selection that is not accepted
// at all is ba_fwd_select's to report, not this table's.
constexpr ba_seg_verdict ba_seg_fwd_support(const ba_fwd_knobs& k) {
  const ba_fwd_choice c = ba_fwd_select(k);
  if (c.bad_knob || c.variant == BA_FWD_PRODUCTION) return {nullptr, 0};
  const ba_fwd_knobs d;
  const int vals[5] = {k.vpath, k.subt, k.nt, k.nbuf, k.kreg};
  const int dflt[5] = {d.vpath, d.subt, d.nt, d.nbuf, d.kreg};
  // the experiment variants are pinned by KREG and SUBT first (see
  // ba_fwd_select), so name those before the knobs they override
  const int order[5] = {4, 1, 2, 3, 0};
  for (int i = 0; i < 5; ++i)
    if (vals[order[i]] != dflt[order[i]])
      return {BA_FWD_KNOB_SPECS[order[i]].env, vals[order[i]]};
  return {nullptr, 0};
}

// Backward: the default plan only (dq + split dV/dK kernels).
constexpr ba_seg_verdict ba_seg_bwd_support(const ba_bwd_knobs& k) {
  if (k.fused) return {BA_BWD_KNOB_SPECS[0].env, k.fused};
  if (k.dk_flip) return {BA_BWD_KNOB_SPECS[1].env, k.dk_flip};
  if (k.dq_pipe) return {BA_BWD_KNOB_SPECS[2].env, k.dq_pipe};
  return {nullptr, 0};
}

// ---- pre-pass workspace --------------------------------------------------
// The kernels stream one side in 64-row tiles while a workgroup owns 256
// rows of the other.  For each (owning, streamed) pair the pre-pass writes
// the (min, max) id of every streamed tile and, per owning block, the
// [lo, hi) range of streamed tiles whose (min, max) overlaps the block's.
// The forward and the dq kernel own q and stream kv; dK/dV own kv and
// stream q.  One workspace holds both pairs, in 32-bit words:
//   flags        [2][B]            streamed ids decrease somewhere: kv, q
//   kv_tile_mm   [B][tiles(Sk)][2]
//   q_blk_range  [B][blocks(Sq)][2]
//   q_tile_mm    [B][tiles(Sq)][2]
//   kv_blk_range [B][blocks(Sk)][2]
constexpr int BA_SEG_TILE = 64;
constexpr int BA_SEG_BLOCK = 256;
constexpr int64_t ba_seg_tiles(int64_t S) {
  return (S + BA_SEG_TILE - 1) / BA_SEG_TILE;
}
constexpr int64_t ba_seg_blocks(int64_t S) {
  return (S + BA_SEG_BLOCK - 1) / BA_SEG_BLOCK;
}
struct ba_seg_ws_layout {
  int64_t flags_kv, flags_q, kv_tile_mm, q_blk_range, q_tile_mm, kv_blk_range,
      words;
};
constexpr ba_seg_ws_layout ba_seg_ws(int64_t B, int64_t Sq, int64_t Sk) {
  ba_seg_ws_layout w{};
  w.flags_kv = 0;
  w.flags_q = B;
  w.kv_tile_mm = 2 * B;  // even: the pairs stay 8-byte aligned
  w.q_blk_range = w.kv_tile_mm + 2 * B * ba_seg_tiles(Sk);
  w.q_tile_mm = w.q_blk_range + 2 * B * ba_seg_blocks(Sq);
  w.kv_blk_range = w.q_tile_mm + 2 * B * ba_seg_tiles(Sq);
  w.words = w.kv_blk_range + 2 * B * ba_seg_blocks(Sk);
  return w;
}
constexpr int64_t ba_seg_ws_bytes(int64_t B, int64_t Sq, int64_t Sk) {
  return ba_seg_ws(B, Sq, Sk).words * 4;
}
