// FP8 (OCP e4m3) forward: a kernel set of its own on the K = 64 scaled MFMA
// (v_mfma_scale_f32_32x32x64_f8f6f4), head_dim 128, forward only.
//
// Work split.  4 waves per workgroup at one wave per SIMD, 128 q rows per
// workgroup (32 per wave), 64-row kv tiles.  K row-major [64][128 B] and the
// permuted V^T image [128][64 B] are double buffered in LDS: 2 x (8 + 8) KiB
// = 32 KiB.  The tile is not made larger: a 64-row tile is exactly one PV
// instruction deep (below), and 32 KiB leaves room for more than one
// workgroup per CU, which this kernel needs more than longer tiles because
// its critical path is the per-score exp / convert work, not the MFMAs.
//
// Operand layout of the K = 64 instruction.  fp8_mfma_probe_kernel
// (probes.hip) establishes three things: lane l holds, as A, row l & 31 and,
// as B, column l & 31; the C/D layout is that of every 32x32 MFMA (ba_crow);
// and A and B use the SAME map from (lane half hi = l >> 5, byte j of the 8
// operand dwords) to contraction index.  It loads both operands under one
// (hi, j) -> k map, and a product is unchanged by a common permutation of k,
// so WHICH index a byte is (the ISA's 32 hi + j) it does not establish.  The
// kernel needs no more than the three: any 32 bytes may stand for the 32
// indices of a half as long as both operands order them alike.
//
// QK.  S^T = mfma(K, Q), two instructions per 32x32 score block (d = 0..63,
// 64..127), unit E8M0 scales (127).  Q fragments stay resident: 2 x 8 dwords.
// The products of two e4m3 values are exact in fp32.
//
// Softmax.  Exp2 domain: one multiplier c2 = sq * sk * softmax_scale *
// log2(e) on the raw scores.  Running (m, l) in fp32 from the unquantised P,
// defer-max with threshold BA_FP8_DEFER_THR: the attn_common.h state
// contract, so state init, finalize and the ring's merge are the D = 128
// ones.
//
// P quantisation.  P <= 2^BA_FP8_DEFER_THR under defer-max.  P is multiplied
// by the power of two BA_FP8_PSCALE = c and rounded to e4m3 (nearest even) by
// v_cvt_pk_fp8_f32.  c * 2^THR = 16 * 16 = 256 <= 448, the largest e4m3, so
// the conversion never saturates; c as large as that bound allows keeps small
// probabilities out of the subnormals (normal down to 2^-6 / c = 2^-10,
// flushed to zero below 2^-10 / c = 2^-14).
//
// PV.  O^T += mfma(V^T, P8^T): ONE K = 64 instruction per 32 v channels and
// kv tile.  A lane's 32 S^T values of a tile (two 32-row sub-blocks kvs, 16
// accumulator registers r each) become, in that order, the 32 bytes of its B
// operand: byte j = 16 kvs + r of lane half hi is kv row
//     ba_fp8_kv_of(hi, j) = 32 kvs + (r & 3) + 8 (r >> 2) + 4 hi
// of the tile.  No lane exchange (the 16-bit kernels need 8 permlane swaps
// per tile here).  The V^T image is laid out under the same permutation: row
// d of a tile's block holds V[kv0 + ba_fp8_kv_of(p >> 5, p & 31)][d] at byte
// p, so a lane's A operand is the 32 bytes [32 hi, 32 hi + 32) of row d.
//
// Descale of V and 1 / c.  The accumulator is kept in units of sv / c for the
// whole call: a carry-in accumulator is multiplied by c / sv when it is
// loaded and the result by sv / c when it is stored.  Applying sv / c per
// tile instead would cost 64 fp32 multiply-adds per lane and tile on the
// path that bounds this kernel; the two extra roundings per call are 2^-24
// relative against the 2^-4 of P.  c is a power of two, and so is sv in the
// exact-P tests: there the round trip is exact.  acc = 0 stays 0.
//
// LDS images and banks (64 banks x 4 B = a 256-byte window of 16 slots;
// ds_read_b128 / ds_write_b128 serve 16 lanes per pass).  Host-side
// enumeration, not a counter run.
//   K: 128-byte rows = 8 slots, so rows r and r + 1 fill one window.  16-byte
//   XOR swizzle slot ^= (row >> 1) & 7.  A 16-lane pass reads rows 16 g ..
//   16 g + 15 at one column slot c: window slot 8 (row & 1) + (c ^ (row >> 1
//   & 7)) is a bijection over the 16 rows: conflict-free, for both reads of
//   the 32-byte operand (slots c and c ^ 1).  A staging pass writes two whole
//   rows, 16 distinct slots.
//   V^T: 64-byte rows = 4 slots, 4 rows per window.  Swizzle slot ^= (row >>
//   2) & 3.  A pass reads rows 16 g .. +15 at slot s = 2 hi + e: window slot
//   4 (row & 3) + (s ^ (row >> 2 & 3)) is a bijection: conflict-free.  The
//   operand's two 16-byte slots always share one aligned 32-byte pair of the
//   row (the XOR may swap their places in it and the pairs of the two lane
//   halves); they are two ds_read_b128.  A staging pass writes four whole
//   rows.
//   Unswizzled, both reads would be 8-way (K) and 4-way (V^T) conflicts.
//
// Block-scaled form (ba_fp8_scale_args in the kernel's trailing pack; an empty
// pack is the per-tensor kernel above, text for text).  Real values are
// q8 * dq[row], k8 * dk[kv tile], v8 * dv[channel]:
//   dq: a lane of S^T owns one q row, so dq[row] folds into that lane's exp2
//   multiplier once per call: c2 = softmax_scale * log2(e) * dq[row].
//   dk: one value per 64-row kv tile, multiplied into c2 for that tile.  The
//   scale is positive, so the row max of the raw scores of ONE tile still
//   commutes with it; across tiles m lives in real exp2 units as before.  The
//   value of tile t + 1 is fetched with tile t + 1's staging loads, one tile
//   ahead of its use, and handed on in a register: no tile waits on it.
//   dv: one value per v channel of this call.  The accumulator row of channel
//   d is kept in units of dv[d] / c for the whole call: the carry-in value is
//   multiplied by c / dv[d], the result by dv[d] / c.  The 128 quotients
//   c / dv[d] are formed once per workgroup, in LDS (512 bytes behind the tile
//   buffers), not 64 divisions per lane; after the loop the same 512 bytes
//   hold dv[d] / c for the store.  Nothing of dv is per tile.
// (acc, m, l) stay fp32 in real units, so rounds with different scales merge.
// The scales must be positive and finite; the quantiser (attn_fp8_quant.hip)
// writes no other.
//
// No segment-id, band, soft-capped, block, module or experiment-variant form
// exists here: the entry points refuse those.
#pragma once
#include "attn_common.h"
#include "attn_host.h"

// The scale tensors of a block-scaled call, fp32, innermost stride 1:
// dq [B][N][Sq], dk [B][Nk][>= k_tile0 + ceil(Sk/64)], dv [B][Nk][128].
// k_tile0 is the dk index of the call's first kv tile.
struct ba_fp8_scale_args {
  const float* dq;
  const float* dk;
  const float* dv;
  int64_t dq_sb, dq_sh;  // batch / head strides in elements
  int64_t dk_sb, dk_sh;
  int64_t dv_sb, dv_sh;
  int k_tile0;
};
__device__ __forceinline__ ba_fp8_scale_args ba_fp8_scale_of(
    const ba_fp8_scale_args& s) {
  return s;
}

constexpr int BA_FP8_D = 128;      // head_dim, q/k/v/o alike
constexpr int BA_FP8_BLOCK = 128;  // q rows a workgroup owns (4 waves x 32)
constexpr int BA_FP8_NT = 256;     // threads per workgroup
constexpr int BA_FP8_KVBLK = 64;   // kv rows per tile = one PV instruction
// P scale c and defer-max threshold: c * 2^THR <= 448 (see above)
constexpr float BA_FP8_PSCALE = (float)BAHIP_F8_P_SCALE;
constexpr float BA_FP8_DEFER_THR = 4.f;
static_assert(BAHIP_F8_P_SCALE * 16 <= 448, "c * 2^THR must stay in e4m3");
constexpr int BA_FP8_E8M0_ONE = 127;  // the E8M0 scale 2^0

typedef __attribute__((ext_vector_type(8))) int i32x8_t;

// kv row (inside its 64-row tile) at byte j of lane half hi of the PV
// operands, and byte position of a kv row in a V^T image row: the inverse
__host__ __device__ constexpr int ba_fp8_kv_of(int hi, int j) {
  return 32 * (j >> 4) + (j & 3) + 8 * ((j & 15) >> 2) + 4 * hi;
}
__host__ __device__ constexpr int ba_fp8_pos_of(int kv) {
  const int r = ((kv & 31) & 3) + 4 * ((kv & 31) >> 3);
  return 32 * ((kv >> 2) & 1) + 16 * (kv >> 5) + r;
}
// the pre-pass builds the image with ba_fp8_kv_of; that it is a permutation
// of the tile's 64 rows, with ba_fp8_pos_of its inverse, is checked here
constexpr bool ba_fp8_perm_ok() {
  for (int p = 0; p < BA_FP8_KVBLK; ++p) {
    const int kv = ba_fp8_kv_of(p >> 5, p & 31);
    if (kv < 0 || kv >= BA_FP8_KVBLK || ba_fp8_pos_of(kv) != p) return false;
  }
  return true;
}
static_assert(ba_fp8_perm_ok(), "ba_fp8_kv_of must permute the 64 kv rows");

// V^T image of a call: [B][Nk][ceil(Sk/64)][128][64] bytes
constexpr int64_t ba_fp8_tiles(int64_t Sk) {
  return (Sk + BA_FP8_KVBLK - 1) / BA_FP8_KVBLK;
}
constexpr int64_t ba_fp8_ws_bytes(int64_t B, int64_t Sk, int64_t Nk) {
  return B * Nk * ba_fp8_tiles(Sk) * BA_FP8_D * BA_FP8_KVBLK;
}

// LDS byte offsets of 16-byte slot `slot` of a row of the two images
__device__ __forceinline__ int ba_fp8_k_off(int row, int slot) {
  return row * 128 + ((slot ^ ((row >> 1) & 7)) << 4);
}
__device__ __forceinline__ int ba_fp8_vt_off(int row, int slot) {
  return row * 64 + ((slot ^ ((row >> 2) & 3)) << 4);
}
// the 32-byte MFMA operand of a lane: slots `slot` and `slot + 1` (slot even)
__device__ __forceinline__ i32x8_t ba_fp8_join(const u32x4_t& a,
                                               const u32x4_t& b) {
  return i32x8_t{(int)a.x, (int)a.y, (int)a.z, (int)a.w,
                 (int)b.x, (int)b.y, (int)b.z, (int)b.w};
}
__device__ __forceinline__ i32x8_t ba_fp8_ld_k(const char* img, int row,
                                               int slot) {
  return ba_fp8_join(*(const u32x4_t*)(img + ba_fp8_k_off(row, slot)),
                     *(const u32x4_t*)(img + ba_fp8_k_off(row, slot + 1)));
}
__device__ __forceinline__ i32x8_t ba_fp8_ld_vt(const char* img, int row,
                                                int slot) {
  return ba_fp8_join(*(const u32x4_t*)(img + ba_fp8_vt_off(row, slot)),
                     *(const u32x4_t*)(img + ba_fp8_vt_off(row, slot + 1)));
}

// d += a * b over 64 e4m3 values per lane row / column, unit scales
__device__ __forceinline__ f32x16_t ba_fp8_mma(const i32x8_t& a,
                                               const i32x8_t& b,
                                               const f32x16_t& c) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
      a, b, c, 0, 0, 0, BA_FP8_E8M0_ONE, 0, BA_FP8_E8M0_ONE);
}

// four fp32 -> one dword of four e4m3 (round to nearest even), byte order
// a, b, c, d
__device__ __forceinline__ int ba_fp8_pack4(float a, float b, float c,
                                            float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  return __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
}
