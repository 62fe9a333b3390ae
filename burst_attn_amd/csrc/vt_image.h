// Layout of the V^T image the forward kernel can stage from instead of V.
//
// One contiguous block per (batch, kv head, 64-row kv tile), each block the
// tile transposed: [B][Nk][ceil(Sk/64)][D][64] elements.  Block (b, nkv, t)
// holds V[b, 64 t + c, nkv, d] at [d][c]; columns with 64 t + c >= Sk (the
// pad of the last tile) are zero.  The block is plain: the LDS swizzle is
// applied where the forward kernel writes it to LDS.  A pre-pass kernel
// (attn_vt_image_kernel in attn_fwd.hip) writes the image once per forward
// call; the forward kernel then copies whole 16-byte chunks of a block.
//
// Host-only and free of HIP includes, so a plain C++17 compiler can build
// it (tests/test_vt_image_cpu.py does).  The kernels and the host launcher
// both take their arithmetic from here.
#pragma once
#include <stdint.h>

constexpr int BA_VT_KVBLK = 64;  // kv rows per block = the forward's KVBLK

// kv tiles (blocks per head) of a Sk-row V
constexpr int64_t ba_vt_tiles(int64_t Sk) {
  return (Sk + BA_VT_KVBLK - 1) / BA_VT_KVBLK;
}
// elements in one block, and the image's head and batch strides in elements
constexpr int64_t ba_vt_block_elems(int64_t D) { return D * BA_VT_KVBLK; }
constexpr int64_t ba_vt_head_stride(int64_t Sk, int64_t D) {
  return ba_vt_tiles(Sk) * ba_vt_block_elems(D);
}
constexpr int64_t ba_vt_batch_stride(int64_t Nk, int64_t Sk, int64_t D) {
  return Nk * ba_vt_head_stride(Sk, D);
}
// byte size of the whole image (elem_bytes = 2 for fp16 and bf16)
constexpr int64_t ba_vt_bytes(int64_t B, int64_t Nk, int64_t Sk, int64_t D,
                              int64_t elem_bytes = 2) {
  return B * ba_vt_batch_stride(Nk, Sk, D) * elem_bytes;
}
// whether a workspace of ws_bytes holds the image: the launcher's check
// (it fails the call, nothing is launched) before the pre-pass writes
constexpr bool ba_vt_workspace_fits(int64_t ws_bytes, int64_t B, int64_t Nk,
                                    int64_t Sk, int64_t D,
                                    int64_t elem_bytes = 2) {
  return ws_bytes >= ba_vt_bytes(B, Nk, Sk, D, elem_bytes);
}
// element offset of V[b, kv, nkv, d] in the image
constexpr int64_t ba_vt_offset(int64_t Nk, int64_t Sk, int64_t D, int64_t b,
                               int64_t nkv, int64_t kv, int64_t d) {
  return b * ba_vt_batch_stride(Nk, Sk, D) + nkv * ba_vt_head_stride(Sk, D) +
         (kv / BA_VT_KVBLK) * ba_vt_block_elems(D) + d * BA_VT_KVBLK +
         kv % BA_VT_KVBLK;
}

// The auto rule (BA_FWD_VT unset): every V tile is staged by
// ceil(Sq/256) * G workgroups (G = q heads per kv head), so that product is
// how often the in-kernel transpose repeats what the pre-pass does once.
// The image path is taken from BA_VT_AUTO_MIN_REUSE upwards; the constant is
// the measured crossover recorded in profiles/fwd_vt/README.md (M4: at
// Sk = 65536, h = 32, d = 128 the image path is 1.7 to 3.2 % slower at a
// reuse of 1 to 8 with G = 1, and not slower at 16 and above).
constexpr int64_t BA_VT_AUTO_MIN_REUSE = 16;
constexpr int64_t ba_vt_reuse(int64_t Sq, int64_t G) {
  return (Sq + 255) / 256 * G;
}
