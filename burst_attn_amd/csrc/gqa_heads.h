// Grouped-query head mapping shared by the forward and backward launchers.
//
// q has N heads, k/v have Nk; query head h attends KV head h / G with
// G = N / Nk (the flash-attn convention).  Host-only and free of HIP
// includes, so a plain C++17 compiler can build it
// (tests/test_gqa_heads_cpu.py does).
#pragma once
#include <stdint.h>

// Group size G for (N, Nk), or 0 when the pair is not a valid grouping
// (Nk < 1, N < Nk, or N not a multiple of Nk).
constexpr int64_t ba_gqa_group(int64_t N, int64_t Nk) {
  return (Nk >= 1 && N >= Nk && N % Nk == 0) ? N / Nk : 0;
}

// KV head of query head n — what the kernels compute once per workgroup.
constexpr int64_t ba_gqa_kv_head(int64_t n, int64_t G) { return n / G; }
