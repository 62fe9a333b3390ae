// head_dim 256: a kernel set of its own at ONE WAVE PER SIMD.
//
// The D = 64/128 kernels run 8 waves per workgroup at two waves per SIMD
// (256 VGPRs each) and are register- and LDS-full at D = 128; 256-wide
// heads double every per-lane accumulator and fragment array and every LDS
// tile.  These kernels therefore run 4 waves per workgroup, one workgroup
// per CU, each wave on the 512-register budget (VGPRs + AGPRs), with the
// resident operands in registers and smaller streamed tiles in LDS:
//
//   forward  128 q rows / workgroup, 64-row kv tiles: K row-major + V^T,
//            double buffered (128 KiB); O accumulator (128) and Q
//            fragments (64) resident
//   dq       128 q rows / workgroup, 32-row kv tiles: K, V, K^T, double
//            buffered (96 KiB); Q and dO fragments (64 + 64) and the dQ^T
//            accumulator (128) resident
//   dV / dK  128 kv rows / workgroup, 32-row q tiles: Q + dO^T (dV, 64 KiB)
//            or Q + dO + Q^T (dK, 96 KiB), double buffered, with the tile's
//            lse*log2e and delta rows behind them; K (and V for dK)
//            fragments and a 128-register accumulator resident
//
// Operand scheme, softmax and state contract are those of attn_common.h and
// attn_fwd.hip (S^T = mfma(K, Q), exp2 domain with defer-max, state =
// (unnormalised acc, m in the exp2 domain, l) with BA_NEG_BIG as the empty
// level), so finalize, state init and the ring's merge serve both sets.
// No segment-id, band, module or experiment-variant form exists here: the
// entry points refuse those at D = 256 (attn_fwd.hip / attn_bwd.hip).  The
// soft-capped form does: each kernel takes one ba_cap_args in a trailing pack.
#pragma once
#include "attn_common.h"
#include "attn_host.h"

constexpr int BA_D256 = 256;
constexpr int BA_D256_BLOCK = 128;  // rows a workgroup owns (4 waves x 32)
constexpr int BA_D256_NT = 256;     // threads per workgroup

// 64-byte image rows (the transposed images of 32-row tiles: K^T, Q^T,
// dO^T).  ba_swz's row >> 3 term leaves two of the four 16-byte slots of
// such a row unused by a 16-lane row-slice read (rows r, r+4, r+8, r+12
// share a 64-byte bank window and must differ in slot), so these images
// take row >> 2, and row >> 4 on top so that the staging scatter (rows 8
// apart across lanes) spreads over all four slots as well.
__device__ __forceinline__ int ba_swz64(int byte, int row) {
  return byte ^ ((((row >> 2) ^ (row >> 4)) & 3) << 4);
}
// ba_ld_rowslice / ba_st_transposed for a [rows][32] image of 64-byte rows
template <typename T>
__device__ __forceinline__ typename mfma_traits<T>::frag ba_ld_rowslice64(
    const T* lds, int row, int elem0) {
  const int byte = ba_swz64(row * 64 + 2 * elem0, row);
  u32x4_t wv = *(const u32x4_t*)((const char*)lds + byte);
  return __builtin_bit_cast(typename mfma_traits<T>::frag, wv);
}
template <typename T>
__device__ __forceinline__ void ba_st_transposed64(T* lds, int src_row, int d0,
                                                   const u32x4_t& chunk) {
  const T* e = (const T*)&chunk;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = d0 + j;
    *(T*)((char*)lds + ba_swz64(row * 64 + 2 * src_row, row)) = e[j];
  }
}

// Launchers (attn_d256_fwd.hip / attn_d256_bwd.hip).  The callers have
// validated shapes, heads and knobs; dtype is BAHIP_F16 or BAHIP_BF16.
int ba_d256_fwd(const fwd_args& a, int out_state, int64_t B, int dtype,
                hipStream_t stream);
int ba_d256_bwd(const bwd_dq_args& dq, const bwd_dq_args& dv,
                const bwd_dq_args& dk, int64_t B, int dtype,
                hipStream_t stream);
// the same in the soft-capped form (attn_common.h, cap_support.h)
int ba_d256_fwd_cap(const fwd_args& a, const ba_cap_args& cp, int out_state,
                    int64_t B, int dtype, hipStream_t stream);
int ba_d256_bwd_cap(const bwd_dq_args& dq, const bwd_dq_args& dv,
                    const bwd_dq_args& dk, const ba_cap_args& cp, int64_t B,
                    int dtype, hipStream_t stream);
