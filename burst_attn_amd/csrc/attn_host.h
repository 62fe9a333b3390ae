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
