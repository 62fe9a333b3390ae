// Host-side helpers shared by the C-ABI entry points in attn_fwd.hip,
// attn_bwd.hip and probes.hip: the last-error message, env knobs, launch
// status, and the (head_dim, dtype) -> <T, D> dispatch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/burst_attn_hip.h"
#include "alibi_support.h"
#include "blk_support.h"
#include "cap_support.h"

// One message buffer for both translation units (C++17 inline variable);
// bahip_last_error() in attn_fwd.hip returns it.
inline thread_local char ba_g_err[256] = "";

// Every nonzero return goes through ba_fail, every zero return through
// ba_ok, so bahip_last_error() never reports an earlier call's message.
__attribute__((format(printf, 2, 3))) inline int ba_fail(int code,
                                                         const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(ba_g_err, sizeof ba_g_err, fmt, ap);
  va_end(ap);
  return code;
}
inline int ba_ok() {
  ba_g_err[0] = '\0';
  return 0;
}

// Knobs are read per call (getenv is ~ns against ms-scale launches) so
// tests can flip variants and plans in-process.
inline int ba_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// status of the launch(es) just issued
inline int ba_launch_status() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return ba_fail((int)e, "kernel launch failed: %s", hipGetErrorString(e));
  return ba_ok();
}
#define BA_CHECK_LAUNCH()                          \
  do {                                             \
    if (int rc_ = ba_launch_status()) return rc_;  \
  } while (0)

// Segment-id pre-pass (defined in attn_fwd.hip, layout in seg_support.h):
// tile summaries of the streamed side `str` and, per 256-row block of the
// owning side `own`, the range of streamed tiles to visit.  The three
// outputs are the workspace regions of that side pair.
int ba_seg_prepass(const int32_t* own, int64_t own_sb, int64_t S_own,
                   const int32_t* str, int64_t str_sb, int64_t S_str,
                   int64_t B, int32_t* flags, int32_t* tile_mm,
                   int32_t* blk_range, hipStream_t stream);

// explicit-kernarg segment size of a kernel, from its parameter types
template <typename F>
struct kernarg_size;
template <typename... P>
struct kernarg_size<void (*)(P...)> {
  static constexpr size_t value = [] {
    size_t off = 0;
    ((off = (off + alignof(P) - 1) / alignof(P) * alignof(P) + sizeof(P)), ...);
    return off;
  }();
};

// ---- launch argument lists shared by the kernel files ---------------------
// One field per attn_fwd_kernel parameter, in kernel order.  launch_fwd
// expands it into the <<<>>> call; the module-launched path hands it to
// the runtime as the packed kernarg buffer (explicit arguments only: the
// HIP runtime appends the hidden ones itself — verified by tools/asm_probe).
// The head_dim 256 forward (attn_d256_fwd.hip) takes the same list.
struct fwd_args {
  const void *q, *k, *v;
  float *o, *lse;
  int Sq, Sk, N, G;
  int64_t q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, v_sb, v_ss, v_sh;
  float scale;
  int causal;
  float *st_acc, *st_m, *st_l;
  int64_t a_sb, a_ss, a_sh, ml_sb, ml_sh;
  int carry_in;
};

// One field per parameter of bwd_dq_kernel and bwd_dkv_kernel (they take the
// same list: the inputs, one fp32 accumulator — dq; dv for MODE 0, dk for
// MODE 1 — and its strides), in kernel order.  The head_dim 256 backward
// kernels (attn_d256_bwd.hip) take it too.
struct bwd_dq_args {
  const void *dout, *q, *k, *v;
  const float *delta, *lse;
  float* out;
  int Sq, Sk, N, G;
  int64_t g_sb, g_ss, g_sh, q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, v_sb, v_ss,
      v_sh, d_sb, d_sh, l_sb, l_sh, o_sb, o_ss, o_sh;
  float scale;
  int causal;
};

// Soft-capped form of the D = 64/128 kernels (cap_support.h): the default
// forward variant and the default backward plan's three kernels, instantiated
// and launched in attn_fwd_softcap.hip / attn_bwd_softcap.hip, which are built
// without packed fp32 VALU ops.  The callers have validated shapes, heads and
// knobs.
int ba_cap_fwd(const fwd_args& a, const ba_cap_args& cp, int out_state,
               int64_t B, int64_t D, int dtype, hipStream_t stream);
int ba_cap_bwd(const bwd_dq_args& dq, const bwd_dq_args& dv,
               const bwd_dq_args& dk, const ba_cap_args& cp, int64_t B,
               int64_t D, int dtype, hipStream_t stream);

// ALiBi form of the D = 64/128 kernels (alibi_support.h): what a *_alibi entry
// point adds to the plain call, and the launches of the default forward
// variant and the default backward plan's three kernels (attn_fwd_alibi.hip /
// attn_bwd_alibi.hip, built without packed fp32 VALU ops).  The callers have
// validated shapes, heads, knobs and the position range.
struct ba_alibi_call {
  const float* slopes;
  int64_t batch_stride, offset, stride;
};
int ba_alibi_fwd(const fwd_args& a, const ba_alibi_args& al, int out_state,
                 int64_t B, int64_t D, int dtype, hipStream_t stream);
int ba_alibi_bwd(const bwd_dq_args& dq, const bwd_dq_args& dv,
                 const bwd_dq_args& dk, const ba_alibi_args& al, int64_t B,
                 int64_t D, int dtype, hipStream_t stream);

// Block form of the D = 64/128 kernels (blk_support.h): what a *_blk entry
// point adds to the plain call, its validation, the pre-pass and the launches
// of the default forward variant and the default backward plan's three
// kernels (attn_fwd_blk.hip / attn_bwd_blk.hip, built without packed fp32 VALU
// ops).  The callers have validated shapes, heads and knobs.
struct ba_blk_call {
  const uint8_t* mask;  // [Bm][Hm][ceil(Sq / BS)][ceil(Sk / BS)], nonzero = set
  int64_t ms[4];        // its element strides
  int64_t Bm, Hm;
  int log2_bs;
  void* ws;
  int64_t ws_bytes;
};
inline int ba_blk_check(const ba_blk_call& c, int64_t B, int64_t Nk,
                        int64_t Sq, int64_t Sk) {
  if (!c.mask)
    return ba_fail(BAHIP_ERR_BLOCK_MASK, "block mask: the mask is null");
  if (!ba_blk_size_ok(c.log2_bs))
    return ba_fail(BAHIP_ERR_BLOCK_MASK,
                   "block mask: the block size must be a power of two >= 64 "
                   "(its log2 was given as %d)",
                   c.log2_bs);
  if (c.Bm != 1 && c.Bm != B)
    return ba_fail(BAHIP_ERR_BLOCK_MASK,
                   "block mask: Bm=%d must be 1 or the batch size B=%d",
                   (int)c.Bm, (int)B);
  if (c.Hm != 1 && c.Hm != Nk)
    return ba_fail(BAHIP_ERR_BLOCK_MASK,
                   "block mask: Hm=%d must be 1 or the KV heads Nk=%d",
                   (int)c.Hm, (int)Nk);
  if (B < 1 || B > 65535 || Nk > 65535 || Sq < 1 || Sk < 1 ||
      Sq > BA_BLK_MAX_S || Sk > BA_BLK_MAX_S)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "block mask: unsupported shape B=%d Sq=%lld Sk=%lld Nk=%d",
                   (int)B, (long long)Sq, (long long)Sk, (int)Nk);
  const int64_t need = ba_blk_ws_bytes(c.Bm, c.Hm, Sq, Sk);
  if (!c.ws || c.ws_bytes < need)
    return ba_fail(BAHIP_ERR_WORKSPACE,
                   "block-mask workspace of %lld bytes is smaller than the "
                   "%lld needed",
                   (long long)(c.ws ? c.ws_bytes : 0), (long long)need);
  return 0;
}
// the lists of the q-owning kernels (q_side), the kv-owning ones (kv_side),
// or both, into c.ws
int ba_blk_prepass(const ba_blk_call& c, int64_t Sq, int64_t Sk, int causal,
                   bool q_side, bool kv_side, hipStream_t stream);
int ba_blk_fwd(const fwd_args& a, const ba_blk_call& c, int out_state,
               int64_t B, int64_t D, int dtype, hipStream_t stream);
int ba_blk_bwd(const bwd_dq_args& dq, const bwd_dq_args& dv,
               const bwd_dq_args& dk, const ba_blk_call& c, int64_t B,
               int64_t D, int dtype, hipStream_t stream);

// f(ba_td<T, D>{}) for the supported (head_dim, dtype) pairs, else 1002.
template <typename T, int D_>
struct ba_td {
  using type = T;
  static constexpr int D = D_;
};
template <typename F>
int ba_dispatch_td(int64_t D, int dtype, F&& f) {
  if (D == 128 && dtype == BAHIP_BF16) return f(ba_td<__bf16, 128>{});
  if (D == 128 && dtype == BAHIP_F16) return f(ba_td<_Float16, 128>{});
  if (D == 64 && dtype == BAHIP_BF16) return f(ba_td<__bf16, 64>{});
  if (D == 64 && dtype == BAHIP_F16) return f(ba_td<_Float16, 64>{});
  return ba_fail(BAHIP_ERR_UNSUPPORTED, "unsupported head_dim %d / dtype %d",
                 (int)D, dtype);
}

// head_dim 256 has a kernel set of its own (attn_d256.h), so it is no row of
// the table above: that table instantiates the D = 64/128 tile kernels, which
// do not fit 256-wide heads.  The small kernels that do (finalize, delta
// preprocess) dispatch here when D == 256.
template <typename F>
int ba_dispatch_t256(int dtype, F&& f) {
  if (dtype == BAHIP_BF16) return f(ba_td<__bf16, 256>{});
  if (dtype == BAHIP_F16) return f(ba_td<_Float16, 256>{});
  return ba_fail(BAHIP_ERR_UNSUPPORTED, "unsupported head_dim 256 / dtype %d",
                 dtype);
}
