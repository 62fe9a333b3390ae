// ALiBi: the argument of the ALiBi form of the kernels and the checks the
// launchers do for it.
//
// With slopes, pair (q row i, kv row j) of the tensors passed gets the score
//   q_i.k_j * softmax_scale - slope[b, h] * |stride * (i - j) + offset|,
// h a QUERY head.  offset and stride place the two tensors in a longer
// sequence: a contiguous piece pair has stride 1 and offset = (first global q
// position) - (first global kv position); a striped pair has stride = world
// size.  The kernels work on raw q.k products, which the softmax scales by
// softmax_scale * log2(e) inside the exp2, so they add the bias in raw units:
//   t = raw + kb * |d|,  kb = -slope / softmax_scale,
// after which max, exp2 and masks are the plain kernel's, bit for bit in
// structure.  d is an int32 per lane and tile, converted once; the 16 scores
// of a lane differ from it by compile-time multiples of stride.
//
// Host-only and free of HIP includes, like band_support.h.
#pragma once
#include <stdint.h>

struct ba_alibi_args {
  const float* slopes;   // [1 or B][N] fp32, head stride 1
  int64_t batch_stride;  // elements between batch rows; 0 = shared
  int32_t offset, stride;
};

// the distance is computed in int32: |offset| + stride * max(Sq, Sk) must
// stay within 2^30, which also leaves room for the rows a tile pads
constexpr int64_t BA_ALIBI_MAX_DIST = (int64_t)1 << 30;
constexpr bool ba_alibi_valid(int64_t offset, int64_t stride, int64_t Sq,
                              int64_t Sk) {
  const int64_t s = Sq > Sk ? Sq : Sk;
  const int64_t ao = offset < 0 ? -offset : offset;
  return stride >= 1 && ao <= BA_ALIBI_MAX_DIST && s >= 0 &&
         stride <= BA_ALIBI_MAX_DIST / (s > 0 ? s : 1) &&
         ao + stride * s <= BA_ALIBI_MAX_DIST;
}
