// FP8 e4m3 quantiser for the block-scaled forward (attn_fp8.h): fp16 / bf16
// [B, S, H, 128] (strided {b, s, h}) -> e4m3 bytes plus the fp32 scale tensor
// of one of three groupings.  x8 = rne(x / scale), scale = amax / 448 of the
// element's group, 1.0 for a group that is all zero: real value = x8 * scale.
//
//   * row mode (q): scale [B][H][S].  One wave per row: a lane holds 2 of the
//     128 channels (one dword), amax by a wave butterfly, 2 bytes out.  One
//     read of the input.
//   * tile mode (k): scale [B][H][ceil(S/64)].  One workgroup (256 threads)
//     per 64-row tile and head: a thread keeps its four 16-byte chunks in
//     registers, the block amax goes wave butterfly -> 4 floats of LDS, then
//     the registers are converted.  Rows past S are neither read nor written.
//     One read.
//   * channel mode (v): scale [B][H][128].  amax per channel over the whole
//     sequence in two launches: partials over 256-row slabs (a thread owns 8
//     channels and every 16th row, 16 x 128 floats of LDS fold the 16 row
//     lanes), then a fold of the slabs' partials, in a fixed order and with
//     no float atomics; a third launch converts.  Two reads.
//
// Conversion is v_cvt_pk_fp8_f32 (round to nearest even) on x * (1 / scale),
// clamped to +-448 first: the quotient of the amax element can land an ulp
// above 448.  The scale is floored at FLT_MIN, so it and its reciprocal are
// positive and finite for every finite input.

#include "attn_fp8.h"

#include <float.h>

namespace {

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;

constexpr int QNT = 256;       // threads per workgroup, every kernel here
constexpr int QD = BA_FP8_D;   // channels per row
constexpr int QCH = QD / 8;    // 16-byte input chunks per row
constexpr int QSLAB = 256;     // rows per partial of the channel mode
constexpr float QMAX = 448.f;  // largest e4m3

template <typename T>
__device__ __forceinline__ float q_elem(unsigned int bits16);
template <>
__device__ __forceinline__ float q_elem<__bf16>(unsigned int b) {
  return __builtin_bit_cast(float, b << 16);
}
template <>
__device__ __forceinline__ float q_elem<_Float16>(unsigned int b) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)b);
}
// the 8 elements of a 16-byte chunk, in memory order
template <typename T>
__device__ __forceinline__ void q_unpack8(const u32x4_t& w, float f[8]) {
  const unsigned int d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = q_elem<T>(d[i] & 0xffffu);
    f[2 * i + 1] = q_elem<T>(d[i] >> 16);
  }
}
__device__ __forceinline__ float q_scale_of(float amax) {
  return amax > 0.f ? fmaxf(amax / QMAX, FLT_MIN) : 1.f;
}
__device__ __forceinline__ float q_clamp(float y) {
  return __builtin_amdgcn_fmed3f(y, -QMAX, QMAX);
}
__device__ __forceinline__ u32x2_t q_pack8(const float f[8], const float inv[8]) {
  return u32x2_t{
      (unsigned int)ba_fp8_pack4(q_clamp(f[0] * inv[0]), q_clamp(f[1] * inv[1]),
                                 q_clamp(f[2] * inv[2]), q_clamp(f[3] * inv[3])),
      (unsigned int)ba_fp8_pack4(q_clamp(f[4] * inv[4]), q_clamp(f[5] * inv[5]),
                                 q_clamp(f[6] * inv[6]),
                                 q_clamp(f[7] * inv[7]))};
}
__device__ __forceinline__ float q_wave_max(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
  return x;
}

struct q_args {
  const char* x;   // input, 2-byte elements
  char* y;         // e4m3 bytes
  float* scale;    // contiguous, layout of the mode
  int S, H;
  int64_t x_sb, x_ss, x_sh;  // elements
  int64_t y_sb, y_ss, y_sh;  // bytes
};

// ---- row mode: grid (ceil(S/4), H, B), wave w of a workgroup owns a row ----
template <typename T>
__global__ __launch_bounds__(QNT) void fp8_quant_row_kernel(q_args a) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * (QNT / 64) + (threadIdx.x >> 6);
  const int h = blockIdx.y, b = blockIdx.z;
  if (s >= a.S) return;  // whole waves leave: no barrier below
  const unsigned int w = *(const unsigned int*)(a.x + 2 * ((int64_t)b * a.x_sb +
      (int64_t)s * a.x_ss + (int64_t)h * a.x_sh) + 4 * lane);
  const float f0 = q_elem<T>(w & 0xffffu), f1 = q_elem<T>(w >> 16);
  const float sc = q_scale_of(q_wave_max(fmaxf(fabsf(f0), fabsf(f1))));
  const float inv = 1.f / sc;
  const int p = __builtin_amdgcn_cvt_pk_fp8_f32(q_clamp(f0 * inv),
                                                q_clamp(f1 * inv), 0, false);
  *(unsigned short*)(a.y + (int64_t)b * a.y_sb + (int64_t)s * a.y_ss +
                     (int64_t)h * a.y_sh + 2 * lane) = (unsigned short)p;
  if (lane == 0) a.scale[((int64_t)b * a.H + h) * a.S + s] = sc;
}

// ---- tile mode: grid (ceil(S/64), H, B) -----------------------------------
template <typename T>
__global__ __launch_bounds__(QNT) void fp8_quant_tile_kernel(q_args a) {
  __shared__ float wmax[QNT / 64];
  const int tid = threadIdx.x;
  const int t = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const char* xp = a.x + 2 * ((int64_t)b * a.x_sb + (int64_t)h * a.x_sh);
  char* yp = a.y + (int64_t)b * a.y_sb + (int64_t)h * a.y_sh;
  const int cc = tid & (QCH - 1);
  float f[4][8];
  float amax = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int row = t * BA_FP8_KVBLK + (tid >> 4) + 16 * c;
    u32x4_t w = {0, 0, 0, 0};
    if (row < a.S)
      w = *(const u32x4_t*)(xp + 2 * ((int64_t)row * a.x_ss) + 16 * cc);
    q_unpack8<T>(w, f[c]);
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(f[c][e]));
  }
  amax = q_wave_max(amax);
  if ((tid & 63) == 0) wmax[tid >> 6] = amax;
  __syncthreads();
  const float sc = q_scale_of(
      fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])));
  const float inv1 = 1.f / sc;
  const float inv[8] = {inv1, inv1, inv1, inv1, inv1, inv1, inv1, inv1};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int row = t * BA_FP8_KVBLK + (tid >> 4) + 16 * c;
    if (row < a.S)
      *(u32x2_t*)(yp + (int64_t)row * a.y_ss + 8 * cc) = q_pack8(f[c], inv);
  }
  if (tid == 0)
    a.scale[((int64_t)b * a.H + h) * gridDim.x + t] = sc;
}

// ---- channel mode ----------------------------------------------------------
// partials: grid (ceil(S/256), H, B) -> part [B][H][slabs][128]
template <typename T>
__global__ __launch_bounds__(QNT) void fp8_quant_chan_part_kernel(
    q_args a, float* __restrict__ part) {
  __shared__ float red[QNT / QCH][QD];
  const int tid = threadIdx.x;
  const int slab = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const char* xp = a.x + 2 * ((int64_t)b * a.x_sb + (int64_t)h * a.x_sh);
  const int cc = tid & (QCH - 1), rl = tid >> 4;
  float am[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r = rl; r < QSLAB; r += QNT / QCH) {
    const int row = slab * QSLAB + r;
    if (row >= a.S) break;
    float f[8];
    q_unpack8<T>(
        *(const u32x4_t*)(xp + 2 * ((int64_t)row * a.x_ss) + 16 * cc), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) am[e] = fmaxf(am[e], fabsf(f[e]));
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[rl][8 * cc + e] = am[e];
  __syncthreads();
  if (tid < QD) {
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < QNT / QCH; ++i) m = fmaxf(m, red[i][tid]);
    part[(((int64_t)b * a.H + h) * gridDim.x + slab) * QD + tid] = m;
  }
}
// final: grid (H, B), 128 threads -> scale [B][H][128]
__global__ __launch_bounds__(QD) void fp8_quant_chan_final_kernel(
    const float* __restrict__ part, float* __restrict__ scale, int slabs) {
  const int64_t bh = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  float m = 0.f;
  for (int i = 0; i < slabs; ++i)
    m = fmaxf(m, part[(bh * slabs + i) * QD + threadIdx.x]);
  scale[bh * QD + threadIdx.x] = q_scale_of(m);
}
// convert: grid (ceil(S/16), H, B), a thread owns one 16-byte chunk of a row
template <typename T>
__global__ __launch_bounds__(QNT) void fp8_quant_chan_cvt_kernel(q_args a) {
  const int tid = threadIdx.x;
  const int row = blockIdx.x * (QNT / QCH) + (tid >> 4);
  const int h = blockIdx.y, b = blockIdx.z;
  const int cc = tid & (QCH - 1);
  if (row >= a.S) return;
  const float* sp = a.scale + ((int64_t)b * a.H + h) * QD + 8 * cc;
  float f[8], inv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) inv[e] = 1.f / sp[e];
  q_unpack8<T>(*(const u32x4_t*)(a.x + 2 * ((int64_t)b * a.x_sb +
      (int64_t)row * a.x_ss + (int64_t)h * a.x_sh) + 16 * cc), f);
  *(u32x2_t*)(a.y + (int64_t)b * a.y_sb + (int64_t)row * a.y_ss +
              (int64_t)h * a.y_sh + 8 * cc) = q_pack8(f, inv);
}

constexpr int64_t q_slabs(int64_t S) { return (S + QSLAB - 1) / QSLAB; }

template <typename T>
int quant_launch(const q_args& a, int mode, int64_t B, float* part,
                 hipStream_t st) {
  const unsigned H = (unsigned)a.H, Bu = (unsigned)B;
  if (mode == BAHIP_F8_QUANT_ROW) {
    fp8_quant_row_kernel<T><<<dim3((a.S + 3) / 4, H, Bu), QNT, 0, st>>>(a);
  } else if (mode == BAHIP_F8_QUANT_TILE) {
    fp8_quant_tile_kernel<T>
        <<<dim3((unsigned)ba_fp8_tiles(a.S), H, Bu), QNT, 0, st>>>(a);
  } else {
    const unsigned slabs = (unsigned)q_slabs(a.S);
    fp8_quant_chan_part_kernel<T><<<dim3(slabs, H, Bu), QNT, 0, st>>>(a, part);
    BA_CHECK_LAUNCH();
    fp8_quant_chan_final_kernel<<<dim3(H, Bu), QD, 0, st>>>(part, a.scale,
                                                            (int)slabs);
    BA_CHECK_LAUNCH();
    fp8_quant_chan_cvt_kernel<T>
        <<<dim3((a.S + QNT / QCH - 1) / (QNT / QCH), H, Bu), QNT, 0, st>>>(a);
  }
  return ba_launch_status();
}

}  // namespace

extern "C" int64_t bahip_attn_quantize_f8_workspace_bytes(int mode, int64_t B,
                                                           int64_t S,
                                                           int64_t H) {
  return mode == BAHIP_F8_QUANT_CHANNEL
             ? B * H * q_slabs(S) * QD * (int64_t)sizeof(float)
             : 0;
}

extern "C" int bahip_attn_quantize_f8(
    const void* x, void* x8, float* scale, int64_t B, int64_t S, int64_t H,
    int64_t D, const int64_t x_strides[3], const int64_t x8_strides[3],
    int dtype, int mode, void* workspace, int64_t workspace_bytes,
    void* stream) {
  if (dtype != BAHIP_F16 && dtype != BAHIP_BF16)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "fp8 quantiser: unsupported input dtype %d (fp16 / bf16)",
                   dtype);
  if (D != QD)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "fp8 quantiser: unsupported head_dim %d (128 only)", (int)D);
  if (mode != BAHIP_F8_QUANT_ROW && mode != BAHIP_F8_QUANT_TILE &&
      mode != BAHIP_F8_QUANT_CHANNEL)
    return ba_fail(BAHIP_ERR_UNSUPPORTED, "fp8 quantiser: unknown mode %d",
                   mode);
  if (B < 1 || B > 65535 || H < 1 || H > 65535 || S < 1 || S > INT32_MAX / 2)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "fp8 quantiser: unsupported shape B=%d S=%lld H=%d", (int)B,
                   (long long)S, (int)H);
  if (!x || !x8 || !scale)
    return ba_fail(BAHIP_ERR_DESCALE,
                   "fp8 quantiser: input, output and scale must be given");
  if ((uintptr_t)x % 16 || (uintptr_t)x8 % 16)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "fp8 quantiser: base pointers must be 16-byte aligned");
  for (int j = 0; j < 3; ++j)
    if (x_strides[j] % 8 || x8_strides[j] % 16)
      return ba_fail(BAHIP_ERR_UNSUPPORTED,
                     "fp8 quantiser: input strides must be multiples of 8 "
                     "elements and output strides of 16 bytes (got %lld, %lld)",
                     (long long)x_strides[j], (long long)x8_strides[j]);
  const int64_t need = bahip_attn_quantize_f8_workspace_bytes(mode, B, S, H);
  if (need && (!workspace || workspace_bytes < need))
    return ba_fail(BAHIP_ERR_WORKSPACE,
                   "fp8 quantiser: workspace of %lld bytes is smaller than "
                   "the %lld needed",
                   (long long)(workspace ? workspace_bytes : 0),
                   (long long)need);
  const q_args a = {(const char*)x, (char*)x8, scale, (int)S, (int)H,
                    x_strides[0], x_strides[1], x_strides[2],
                    x8_strides[0], x8_strides[1], x8_strides[2]};
  if (dtype == BAHIP_F16)
    return quant_launch<_Float16>(a, mode, B, (float*)workspace,
                                  (hipStream_t)stream);
  return quant_launch<__bf16>(a, mode, B, (float*)workspace,
                              (hipStream_t)stream);
}
