// Standalone perf bisect for the fused dK+dQ kernel (no torch import —
// seconds per run).  Times each DBG variant of bwd_dkq_kernel plus the
// split-plan kernels on the s=65536 headline shape, so one gpurun call
// pinpoints which component (K^T reads, ds_add reduce, global atomics,
// LDS size, barriers) carries a slowdown.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/dkq_probe.hip -o tools/dkq_probe
#include "../burst_attn_amd/csrc/attn_bwd.hip"

#include <stdio.h>

#define CK(x)                                                        \
  do {                                                               \
    hipError_t e_ = (x);                                             \
    if (e_ != hipSuccess) {                                          \
      printf("HIP error %s @%d\n", hipGetErrorString(e_), __LINE__); \
      return 1;                                                      \
    }                                                                \
  } while (0)

__global__ void fill_kernel(_Float16* p, size_t n, unsigned seed) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    unsigned h = (unsigned)i * 2654435761u + seed;
    h ^= h >> 13;
    p[i] = (_Float16)(((float)(h & 1023) / 512.f) - 1.f);
  }
}
__global__ void fillf_kernel(float* p, size_t n, float v) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

int main(int argc, char** argv) {
  const int B = 1, S = (argc > 1) ? atoi(argv[1]) : 65536, N = 32, D = 128;
  using T = _Float16;
  const size_t nel = (size_t)B * S * N * D;
  T *q, *k, *v, *dout;
  float *delta, *lse, *dq, *dk, *dv2;
  CK(hipMalloc(&q, nel * 2));
  CK(hipMalloc(&k, nel * 2));
  CK(hipMalloc(&v, nel * 2));
  CK(hipMalloc(&dout, nel * 2));
  CK(hipMalloc(&delta, (size_t)B * N * S * 4));
  CK(hipMalloc(&lse, (size_t)B * N * S * 4));
  CK(hipMalloc(&dq, nel * 4));
  CK(hipMalloc(&dk, nel * 4));
  CK(hipMalloc(&dv2, nel * 4));
  int thr = 256;
  fill_kernel<<<(nel + thr - 1) / thr, thr>>>(q, nel, 1);
  fill_kernel<<<(nel + thr - 1) / thr, thr>>>(k, nel, 2);
  fill_kernel<<<(nel + thr - 1) / thr, thr>>>(v, nel, 3);
  fill_kernel<<<(nel + thr - 1) / thr, thr>>>(dout, nel, 4);
  size_t nml = (size_t)B * N * S;
  fillf_kernel<<<(nml + thr - 1) / thr, thr>>>(delta, nml, 0.5f);
  fillf_kernel<<<(nml + thr - 1) / thr, thr>>>(lse, nml, 11.f);
  CK(hipMemset(dq, 0, nel * 4));
  CK(hipMemset(dk, 0, nel * 4));
  CK(hipMemset(dv2, 0, nel * 4));
  CK(hipDeviceSynchronize());

  // attn_bwd.hip's own argument structs: dense tensors, non-causal, G = 1
  const float scale = 0.0883883f;
  const int64_t sb = (int64_t)S * N * D, ss = (int64_t)N * D, sh = D;
  const int64_t lb = (int64_t)N * S, lh = S;
  auto inputs = [&](auto& a) {  // the fields all three structs share
    a.dout = dout, a.q = q, a.k = k, a.v = v, a.delta = delta, a.lse = lse;
    a.Sq = a.Sk = S, a.N = N, a.scale = scale, a.causal = 0;
    a.g_sb = a.q_sb = a.k_sb = a.v_sb = sb;
    a.g_ss = a.q_ss = a.k_ss = a.v_ss = ss;
    a.g_sh = a.q_sh = a.k_sh = a.v_sh = sh;
    a.d_sb = a.l_sb = lb, a.d_sh = a.l_sh = lh;
  };
  bwd_dkq_args dkqa = {};
  inputs(dkqa);
  dkqa.dq = dq, dkqa.dk = dk, dkqa.dv = dv2;
  dkqa.dq_sb = dkqa.dk_sb = dkqa.dv_sb = sb;
  dkqa.dq_ss = dkqa.dk_ss = dkqa.dv_ss = ss;
  dkqa.dq_sh = dkqa.dk_sh = dkqa.dv_sh = sh;
  bwd_dkv_args dkva = {};
  inputs(dkva);
  dkva.G = 1, dkva.out = dk, dkva.o_sb = sb, dkva.o_ss = ss, dkva.o_sh = sh;
  bwd_dq_args dqa = dkva;
  dqa.out = dq;

  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  auto bench = [&](const char* name, auto launch) {
    launch();  // warm
    (void)hipDeviceSynchronize();
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) {
      printf("%-28s LAUNCH ERROR: %s\n", name, hipGetErrorString(le));
      return;
    }
    (void)hipEventRecord(e0);
    launch();
    launch();
    (void)hipEventRecord(e1);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    printf("%-28s %8.2f ms\n", name, ms / 2);
  };

  bench("dkq FUSE0 (flip dK)", [&] { launch_dkq<T, 128, 0, 0, 64>(dkqa, B, 0); });
  bench("dkq FUSE1 DBG0 (full)", [&] { launch_dkq<T, 128, 1, 0, 64>(dkqa, B, 0); });
  bench("dkq FUSE1 DBG1 (noGlbAtom)", [&] { launch_dkq<T, 128, 1, 1, 64>(dkqa, B, 0); });
  bench("dkq FUSE1 DBG2 (dsWrite)", [&] { launch_dkq<T, 128, 1, 2, 64>(dkqa, B, 0); });
  bench("dkq FUSE1 DBG3 (no dQ sec)", [&] { launch_dkq<T, 128, 1, 3, 64>(dkqa, B, 0); });
  bench("dkq FUSE1 DBG4 (no KT rd)", [&] { launch_dkq<T, 128, 1, 4, 64>(dkqa, B, 0); });
  bench("dkq FUSE1 DBG5 (no reduce)", [&] { launch_dkq<T, 128, 1, 5, 64>(dkqa, B, 0); });
  bench("dkq FUSE1 DBG0 SCRW32", [&] { launch_dkq<T, 128, 1, 0, 32>(dkqa, B, 0); });
  bench("dkvf (fused dK+dV)", [&] { launch_dkq<T, 128, 0, 0, 32, 1>(dkqa, B, 0); });
  bench("dkv MODE1 (split dK)", [&] { launch_dkv<T, 128, 1>(dkva, B, 0); });
  bench("dkv MODE0 (dV)", [&] { launch_dkv<T, 128, 0>(dkva, B, 0); });
  bench("dq kernel DQP=1", [&] { launch_dq<T, 128, 1>(dqa, B, 0); });
  bench("dq kernel", [&] { launch_dq<T, 128, 0>(dqa, B, 0); });
  return 0;
}
