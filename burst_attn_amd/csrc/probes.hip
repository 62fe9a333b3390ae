// Hardware-semantics probes (test support): they pin the MFMA lane maps
// and the ds_read_tr16_b64 behaviour that attn_common.h assumes.  Kept out
// of the kernel sources so the forward's .s -> hsaco side-build carries
// attention kernels only.

#include "attn_common.h"
#include "attn_host.h"
#include "probes.h"

namespace {

// ---- MFMA layout probe: D = A*B for one 32x32x16 tile, with A,B,D moved
// per the layout assumptions of attn_common.h.  a: [32][16] row-major,
// b: [16][32] row-major, d: [32][32] row-major, all dense in HBM.
template <typename T>
__global__ void mfma_probe_kernel(const T* a, const T* b, float* d) {
  using MT = mfma_traits<T>;
  using frag = typename MT::frag;
  const int lane = threadIdx.x & 63;
  const int l31 = lane & 31, hi = lane >> 5;
  frag af, bf;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    af[j] = a[l31 * 16 + 8 * hi + j];    // A[row=l31][k=8*hi+j]
    bf[j] = b[(8 * hi + j) * 32 + l31];  // B[k=8*hi+j][col=l31]
  }
  f32x16_t c = (f32x16_t)(0.f);
  c = MT::mma(af, bf, c);
#pragma unroll
  for (int r = 0; r < 16; ++r) d[ba_crow(r, hi) * 32 + l31] = c[r];
}

// ---- ds_read_tr16_b64 semantics probe.
// Fills LDS with element-index pattern, issues the transpose-read with a
// per-mode address pattern, dumps each lane's 4 returned u16s.
__global__ void tr16_probe_kernel(int mode, int* out) {
  __shared__ unsigned short lds[4096];
  for (int i = threadIdx.x; i < 4096; i += 64) lds[i] = (unsigned short)i;
  __syncthreads();
  const int l = threadIdx.x & 63;
  int e;
  switch (mode) {
    case 0: e = 0; break;               // uniform base
    case 1: e = (l & 15) * 4; break;    // per-16-group column stride 4
    case 2: e = l * 4; break;           // per-lane stride 4
    case 3: e = (l >> 4) * 64; break;   // per-quarter base
    default: e = (l & 15) * 4 + (l >> 4) * 256; break;
  }
  auto p = (__attribute__((address_space(3))) s16x4_t*)&lds[e];
  s16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(p);
#pragma unroll
  for (int j = 0; j < 4; ++j) out[l * 4 + j] = (int)(unsigned short)v[j];
}

}  // namespace

extern "C" int bahip_tr16_probe(int mode, int* out, void* stream) {
  tr16_probe_kernel<<<1, 64, 0, (hipStream_t)stream>>>(mode, out);
  return ba_launch_status();
}

extern "C" int bahip_mfma_probe(const void* a, const void* b, float* d,
                                int dtype, void* stream) {
  if (dtype == BAHIP_BF16)
    mfma_probe_kernel<__bf16><<<1, 64, 0, (hipStream_t)stream>>>(
        (const __bf16*)a, (const __bf16*)b, d);
  else
    mfma_probe_kernel<_Float16><<<1, 64, 0, (hipStream_t)stream>>>(
        (const _Float16*)a, (const _Float16*)b, d);
  return ba_launch_status();
}
