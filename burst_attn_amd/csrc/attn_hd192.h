// qk head_dim 192 with v head_dim 128 (multi-head latent attention heads
// after the up-projection: 128 "nope" + 64 rope q/k channels, 128 v/o
// channels): a kernel set of its own at ONE WAVE PER SIMD.
//
// Each kernel has two contraction widths.  q, k, dq, dk are 192 wide; v, o,
// dO, the carry-in accumulator and dv are 128 wide; lse, delta, m, l are per
// row as everywhere.  The split is attn_d256.h's (4 waves per workgroup, one
// workgroup per CU, 128 owned rows, the 512-register budget) with what is
// resident sized by the width it is contracted over or written at:
//
//   forward  128 q rows / workgroup, 64-row kv tiles: K row-major [kv][192]
//            + V^T [128][kv], double buffered (82 KiB); the O^T accumulator
//            (64) and the Q fragments (48) resident
//   dq       128 q rows / workgroup, 32-row kv tiles: K [kv][192], V
//            [kv][128], K^T [192][kv], double buffered (65 KiB); Q (48) and
//            dO (32) fragments and the dQ^T accumulator (96) resident
//   dV       128 kv rows / workgroup, 32-row q tiles: Q [q][192] + dO^T
//            [128][q] (41 KiB); K fragments (48) and a 64-register
//            accumulator resident
//   dK       the same with Q + dO [q][128] + Q^T [192][q] (65 KiB); K (48)
//            and V (32) fragments and a 96-register accumulator resident
//
// Operand scheme, softmax and state contract are those of attn_common.h
// (S^T = mfma(K, Q), exp2 domain with defer-max, P / dS to fragments in
// registers, state = (unnormalised acc, m in the exp2 domain, l) with
// BA_NEG_BIG as the empty level), so state init, finalize and the delta
// preprocess are the existing kernels at D = 128, and the ring's merge
// serves this set too.  No segment-id, band, soft-capped, block, module or
// experiment-variant form exists here: the entry points refuse those.
//
// 192-wide row-major images.  A 384-byte row is 96 banks: 1.5 bank windows
// of 256 bytes.  A 16-byte XOR swizzle can only permute the 8 slots of an
// aligned 128-byte group (slots 16..23 XOR 8 would leave the row), and with
// 3 swizzle bits rows r and r + 8 of a 16-lane ds_read_b128 group land in
// the same slot of the window: row * 24 slots = (row & 1) * 8 mod 16, so the
// window offset has one bit of row in it and the XOR three, 16 slots for 16
// rows is not reachable.  The images are therefore PADDED to 400-byte rows
// and not swizzled: 25 slots per row is odd, so the 16 rows of a lane group
// reading one column land in 16 distinct slots of the window ((25 r + c) mod
// 16 is a bijection in r), all 64 banks, conflict-free, for every column
// and both lane halves.  A staging write of 16 lanes covers two rows' 128
// contiguous bytes, slots s..s+7 and s+9..s+16: one slot of 16 is shared
// (2-way on 4 banks).  Cost: 16 bytes per row, 1 KiB per 64-row tile.  This
// is host-side enumeration, not a counter run.
#pragma once
#include "attn_d256.h"

constexpr int BA_HD192_DQK = 192;    // q/k/dq/dk width
constexpr int BA_HD192_DV = 128;     // v/o/dO/acc/dv width
constexpr int BA_HD192_BLOCK = 128;  // rows a workgroup owns (4 waves x 32)
constexpr int BA_HD192_NT = 256;     // threads per workgroup
constexpr int BA_HD192_ROWB = 400;   // bytes per row of a 192-wide image
// 128-wide row-major images have 256-byte rows: 16 slots, the D = 128
// kernels' swizzle
constexpr int BA_HD192_SWZV = 15;

// 16-byte fragment read / chunk write of a padded 192-wide row-major image
template <typename T>
__device__ __forceinline__ typename mfma_traits<T>::frag ba_ld_row192(
    const char* img, int row, int elem0) {
  u32x4_t wv = *(const u32x4_t*)(img + row * BA_HD192_ROWB + 2 * elem0);
  return __builtin_bit_cast(typename mfma_traits<T>::frag, wv);
}
__device__ __forceinline__ void ba_st_row192(char* img, int row, int col8,
                                             const u32x4_t& chunk) {
  *(u32x4_t*)(img + row * BA_HD192_ROWB + col8 * 16) = chunk;
}

// Staging chunk maps: eight consecutive threads cover 128 contiguous bytes of
// a row, and chunk index c steps the column by 64 elements (and, in the
// forward's 64-row tiles, the row by 32).  Neither step changes a swizzle
// term of any image here, so a thread's LDS write addresses differ by
// constants.  192-wide rows are 24 chunks = 3 column steps, 128-wide rows 16
// = 2: a 32-row tile is 3 (resp. 2) chunks per thread, no thread idles.
struct ba_hd192_rc {
  int row, col8;
};
__device__ __forceinline__ ba_hd192_rc ba_hd192_rc_qk(int c) {
  return {((int)threadIdx.x >> 3) + 32 * (c / 3),
          ((int)threadIdx.x & 7) + 8 * (c % 3)};
}
__device__ __forceinline__ ba_hd192_rc ba_hd192_rc_v(int c) {
  return {((int)threadIdx.x >> 3) + 32 * (c >> 1),
          ((int)threadIdx.x & 7) + 8 * (c & 1)};
}

// f(ba_td<T, 192>{}) for the two dtypes, else BAHIP_ERR_UNSUPPORTED
template <typename F>
int ba_dispatch_t192(int dtype, F&& f) {
  if (dtype == BAHIP_BF16) return f(ba_td<__bf16, BA_HD192_DQK>{});
  if (dtype == BAHIP_F16) return f(ba_td<_Float16, BA_HD192_DQK>{});
  return ba_fail(BAHIP_ERR_UNSUPPORTED,
                 "unsupported head_dim pair (192, 128) / dtype %d", dtype);
}

// What a *_dv entry point does with (D, Dv): 0 = the pair is the new set's,
// 1 = D == Dv, the existing entry point's; else the refusal, message set.
inline int ba_hd192_route(int64_t D, int64_t Dv, int* same) {
  *same = D == Dv;
  if (*same || (D == BA_HD192_DQK && Dv == BA_HD192_DV)) return 0;
  return ba_fail(BAHIP_ERR_UNSUPPORTED,
                 "head_dim mismatch: unsupported head_dim pair qk=%d v=%d "
                 "(equal widths 64/128/256, or qk=192 with v=128)",
                 (int)D, (int)Dv);
}
