// Test-support entry points of probes.hip.  Not part of the C ABI in
// include/burst_attn_hip.h: only the torch binding's mfma_probe /
// tr16_probe call them.  Return codes and bahip_last_error() as there.
#pragma once

#ifdef __cplusplus
extern "C" {
#endif

// d[32][32] = a[32][16] * b[16][32] through one 32x32x16 MFMA; a, b dense
// row-major of `dtype` (BAHIP_F16 / BAHIP_BF16), d fp32.
int bahip_mfma_probe(const void* a, const void* b, float* d, int dtype,
                     void* stream);

// out[64 lanes][4] = what ds_read_tr16_b64 returns for address pattern
// `mode` (0..4) over an LDS image holding its own element indices.
int bahip_tr16_probe(int mode, int* out, void* stream);

#ifdef __cplusplus
}
#endif
