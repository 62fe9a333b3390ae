// FP8 e4m3 forward tile kernel for gfx950 (design: attn_fp8.h), its V^T image
// pre-pass, and the *_f8 entry points.
//
//   * workgroup = 4 waves (256 threads), one per SIMD; wave w owns q rows
//     [blk*128 + w*32, +32); grid = (ceil(Sq/128), N, B).
//   * 64-row kv tiles in LDS, double buffered, one barrier per tile; the
//     next tile's global loads (2 + 2 dwordx4 per thread) are issued before
//     the current tile's MFMAs.  K comes from the caller's tensor, V^T from
//     the image the pre-pass wrote: both are 16-byte copies.
//   * per tile and wave: S^T = mfma(K, Q) for the two 32-row sub-blocks (4
//     K = 64 MFMAs), lane-local online softmax in the exp2 domain with
//     defer-max over all 32 scores of the lane, P -> e4m3 in registers (16
//     v_cvt_pk_fp8_f32), O^T += mfma(V^T, P^T) (4 MFMAs): 8 MFMAs where the
//     16-bit D = 128 kernel issues 32.
//   * resident per lane: the O^T accumulator (4 x 16 fp32) and the Q
//     fragments (2 x 8 dwords).
//   * OUT_STATE as in attn_fwd.hip: 0 = normalised o + lse, 1 = the carry-in
//     / carry-out state (acc, m, l), bit-compatible with the D = 128 kernels'.
//   * SC: empty = per-tensor descales folded into fp8_extra by the host.  One
//     ba_fp8_scale_args = the block-scaled form (attn_fp8.h): dq per q row,
//     dk per kv tile, dv per v channel, read from device tensors.

#include "attn_fp8.h"
#include "fwd_variants.h"
#include "gqa_heads.h"
#include "seg_support.h"

#include <math.h>

namespace {

// One field per attn_fp8_fwd_kernel parameter that fwd_args does not have.
struct fp8_extra {
  const char* vt;   // V^T image of the call
  float c2;         // sq * sk * softmax_scale * log2(e)
  float in_mul;     // c / sv: carry-in accumulator -> kernel units
  float out_mul;    // sv / c: kernel units -> real
};

// ---- V^T image pre-pass: one workgroup per (kv tile, kv head, batch) -------
// reads the tile's 64 x 128 bytes (rows past Sk as zero), writes the block
// [128][64] under the PV permutation (ba_fp8_pos_of)
__global__ __launch_bounds__(BA_FP8_NT) void attn_fp8_vt_kernel(
    const char* __restrict__ v, char* __restrict__ img, int Sk, int Nk,
    int64_t v_sb, int64_t v_ss, int64_t v_sh) {
  constexpr int PITCH = 144;  // 16-byte aligned rows, 36 banks apart
  __shared__ __attribute__((aligned(16))) char raw[BA_FP8_KVBLK * PITCH];
  const int tid = threadIdx.x;
  const int t = blockIdx.x, nkv = blockIdx.y, b = blockIdx.z;
  const char* vp = v + (int64_t)b * v_sb + (int64_t)nkv * v_sh;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int row = (tid >> 3) + 32 * c, col = (tid & 7) * 16;
    const int kv = t * BA_FP8_KVBLK + row;
    u32x4_t w = {0, 0, 0, 0};
    if (kv < Sk) w = *(const u32x4_t*)(vp + (int64_t)kv * v_ss + col);
    *(u32x4_t*)(raw + row * PITCH + col) = w;
  }
  __syncthreads();
  char* blk = img + (((int64_t)b * Nk + nkv) * gridDim.x + t) *
                        (BA_FP8_D * BA_FP8_KVBLK);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int idx = tid + BA_FP8_NT * c;  // 16-byte chunk of the block
    const int d = idx >> 2, s = idx & 3;
    unsigned int w[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      w[g] = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kv = ba_fp8_kv_of(s >> 1, 16 * (s & 1) + 4 * g + e);
        w[g] |= (unsigned int)(unsigned char)raw[kv * PITCH + d] << (8 * e);
      }
    }
    *(u32x4_t*)(blk + idx * 16) = u32x4_t{w[0], w[1], w[2], w[3]};
  }
}

// At least two waves per SIMD: with the default budget the compiler spreads
// 164 + 96 registers over both files, 4 past what two workgroups per CU
// allow; asked for two it needs 167 in all, no AGPRs and no scratch, and
// three workgroups fit a CU (32 KiB of LDS each).
// The scaled form asks for three: its LDS multipliers let the compiler batch
// the epilogue's reads into 185 registers otherwise, one workgroup per CU less.
template <int OUT_STATE, typename... SC>
__global__ __launch_bounds__(BA_FP8_NT, sizeof...(SC) ? 3 : 2) void
attn_fp8_fwd_kernel(
    const char* __restrict__ q, const char* __restrict__ k,
    float* __restrict__ o, float* __restrict__ lse,
    int Sq, int Sk, int N, int G,
    int64_t q_sb, int64_t q_ss, int64_t q_sh,
    int64_t k_sb, int64_t k_ss, int64_t k_sh,
    int causal,
    float* __restrict__ st_acc, float* __restrict__ st_m,
    float* __restrict__ st_l,
    int64_t a_sb, int64_t a_ss, int64_t a_sh,
    int64_t ml_sb, int64_t ml_sh, int carry_in, fp8_extra x, SC... sc) {
  constexpr bool HAS_SC = ba_pack_is<ba_fp8_scale_args, SC...>;
  static_assert(HAS_SC || sizeof...(SC) == 0,
                "the pack: one ba_fp8_scale_args");
  constexpr int D = BA_FP8_D;
  constexpr int NT = BA_FP8_NT;
  constexpr int KVBLK = BA_FP8_KVBLK;
  constexpr int TILEB = KVBLK * D;  // bytes of a K tile and of a V^T block
  constexpr int PT = TILEB / 16 / NT;  // 2 chunks of each per thread

  // [2 buffers][K row-major | V^T], both swizzled (attn_fp8.h); the scaled
  // form keeps the 128 carry-in multipliers c / dv[d] behind them
  __shared__ __attribute__((aligned(16))) char
      lds[2 * 2 * TILEB + (HAS_SC ? D * (int)sizeof(float) : 0)];
  auto ldsK = [&](int buf) -> char* { return lds + buf * 2 * TILEB; };
  auto ldsVT = [&](int buf) -> char* { return lds + buf * 2 * TILEB + TILEB; };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31;
  const int hi = lane >> 5;
  const int n = blockIdx.y;
  const int b = blockIdx.z;
  const int qb = blockIdx.x * BA_FP8_BLOCK + wave * 32;
  const int q_row = qb + l31;
  const int nkv = n / G;  // grouped-query heads: q head n attends n / G
  const int Nk = N / G;
  const int ntiles_all = (Sk + KVBLK - 1) / KVBLK;

  const char* qp = q + (int64_t)b * q_sb + (int64_t)n * q_sh;
  const char* kp = k + (int64_t)b * k_sb + (int64_t)nkv * k_sh;
  const char* vtp = x.vt + ((int64_t)b * Nk + nkv) * ntiles_all * TILEB;

  // Q fragments: B operand of S^T = mfma(K, Q); lane holds q row q_row,
  // channels d = 64 i + 32 hi + [0, 32)
  i32x8_t qf[D / 64];
#pragma unroll
  for (int i = 0; i < D / 64; ++i) {
    u32x4_t w0 = {0, 0, 0, 0}, w1 = {0, 0, 0, 0};
    if (q_row < Sq) {
      const char* p = qp + (int64_t)q_row * q_ss + 64 * i + 32 * hi;
      w0 = *(const u32x4_t*)p;
      w1 = *(const u32x4_t*)(p + 16);
    }
    qf[i] = ba_fp8_join(w0, w1);
  }

  // scaled form: x.c2 is softmax_scale * log2(e) alone; the row's dq joins
  // it here, the tile's dk in the loop
  float c2q = x.c2;
  const float* dkp = nullptr;
  const float* dvp = nullptr;
  float dk_cur = 1.f, dk_next = 1.f;
  if constexpr (HAS_SC) {
    const ba_fp8_scale_args sa = ba_fp8_scale_of(sc...);
    if (q_row < Sq) c2q *= sa.dq[b * sa.dq_sb + n * sa.dq_sh + q_row];
    dkp = sa.dk + b * sa.dk_sb + nkv * sa.dk_sh + sa.k_tile0;
    dvp = sa.dv + b * sa.dv_sb + nkv * sa.dv_sh;
    dk_cur = dkp[0];
    if (OUT_STATE && carry_in) {  // uniform: the whole grid takes one side
      if (tid < D)
        ((float*)(lds + 2 * 2 * TILEB))[tid] = BA_FP8_PSCALE / dvp[tid];
      __syncthreads();
    }
  }
  constexpr float LOG2C = 4.f;  // log2(BA_FP8_PSCALE)
  static_assert(BA_FP8_PSCALE == 16.f, "LOG2C follows BA_FP8_PSCALE");
  float m2 = BA_NEG_BIG;
  float lsum = 0.f;
  f32x16_t ot[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) ot[dt] = (f32x16_t)(0.f);
  if (OUT_STATE && carry_in && q_row < Sq) {
    m2 = st_m[b * ml_sb + n * ml_sh + q_row];
    lsum = st_l[b * ml_sb + n * ml_sh + q_row];
    const float* arow = st_acc + b * a_sb + (int64_t)q_row * a_ss + n * a_sh;
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if constexpr (HAS_SC)
          ot[dt][r] = arow[dt * 32 + ba_crow(r, hi)] *
                      ((const float*)(lds + 2 * 2 * TILEB))[dt * 32 +
                                                           ba_crow(r, hi)];
        else
          ot[dt][r] = arow[dt * 32 + ba_crow(r, hi)] * x.in_mul;
  }

  // causal: no key past the block's last row is visible to any of its rows
  const int kv_limit =
      causal ? min(Sk, (int)(blockIdx.x + 1) * BA_FP8_BLOCK) : Sk;
  const int nt = (kv_limit + KVBLK - 1) / KVBLK;

  auto issue_loads = [&](int tile, u32x4_t* kreg, u32x4_t* vreg) {
    const int kv0 = tile * KVBLK;
    // K rows clamped, not guarded: rows past Sk re-load row Sk - 1 and the
    // kv-range mask gives them p = 0; the image's pad columns are zero
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      const int row = (tid >> 3) + 32 * c;
      const int kvg = kv0 + row;
      const int kvc = kvg < Sk ? kvg : (Sk - 1);
      kreg[c] = *(const u32x4_t*)(kp + (int64_t)kvc * k_ss + (tid & 7) * 16);
      vreg[c] = *(const u32x4_t*)(vtp + (int64_t)tile * TILEB +
                                  (tid + NT * c) * 16);
    }
  };
  auto write_lds = [&](int buf, const u32x4_t* kreg, const u32x4_t* vreg) {
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      *(u32x4_t*)(ldsK(buf) + ba_fp8_k_off((tid >> 3) + 32 * c, tid & 7)) =
          kreg[c];
      const int idx = tid + NT * c;
      *(u32x4_t*)(ldsVT(buf) + ba_fp8_vt_off(idx >> 2, idx & 3)) = vreg[c];
    }
  };

  {
    u32x4_t kreg[PT], vreg[PT];
    issue_loads(0, kreg, vreg);
    write_lds(0, kreg, vreg);
    __syncthreads();
  }

  int cur = 0;
  for (int t = 0; t < nt; ++t) {
    const int kv0 = t * KVBLK;
    const bool has_next = (t + 1) < nt;
    u32x4_t kreg[PT], vreg[PT];
    if (has_next) {
      issue_loads(t + 1, kreg, vreg);
      // the next tile's dk rides with its staging loads, a tile ahead of use
      if constexpr (HAS_SC) dk_next = dkp[t + 1];
    }
    const float c2 = HAS_SC ? c2q * dk_cur : c2q;

    // causal: a tile wholly above the diagonal of this wave's 32 rows
    if (!causal || kv0 <= qb + 31) {
      // S^T = mfma(K, Q) over the 128 channels: raw, unscaled scores of the
      // tile's two 32-row sub-blocks
      f32x16_t s[2];
#pragma unroll
      for (int kvs = 0; kvs < 2; ++kvs) {
        s[kvs] = (f32x16_t)(0.f);
#pragma unroll
        for (int i = 0; i < D / 64; ++i)
          s[kvs] = ba_fp8_mma(
              ba_fp8_ld_k(ldsK(cur), kvs * 32 + l31, 4 * i + 2 * hi), qf[i],
              s[kvs]);
      }
      // a full tile needs no mask: inside Sk and, if causal, at or below
      // the diagonal for every row of this wave
      const bool full =
          (kv0 + KVBLK <= Sk) && (!causal || (kv0 + KVBLK - 1 <= qb));
      if (!full) {
#pragma unroll
        for (int kvs = 0; kvs < 2; ++kvs)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kv_g = kv0 + kvs * 32 + ba_crow(r, hi);
            if (!(kv_g < Sk && (!causal || kv_g <= q_row)))
              s[kvs][r] = BA_NEG_BIG;
          }
      }
      // row max on raw scores (max commutes with c2 > 0, one c2 per tile)
      float tm = fmaxf(ba_max16(s[0]), ba_max16(s[1]));
      {
        float lo, hi2;
        ba_half_pair(tm, lo, hi2);
        tm = fmaxf(lo, hi2) * c2;
      }
      // defer-max: skip the O/l rescale while the running max grows by
      // <= THR, so p <= 2^THR; decided before the scores are exponentiated
      if (!__all(tm - m2 <= BA_FP8_DEFER_THR)) {
        const float mnew = fmaxf(m2, tm);
        const float alpha = ba_exp2(m2 - mnew);
        m2 = mnew;
        lsum *= alpha;
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) ot[dt][r] *= alpha;
      }
      // p * c = exp2(s c2 - (m2 - log2 c)): the scale costs nothing, and the
      // row sum of the unquantised p is that of p * c over c
      const float m2c = m2 - LOG2C;
      float rowsum = 0.f;
#pragma unroll
      for (int kvs = 0; kvs < 2; ++kvs)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s[kvs][r] = ba_exp2(__builtin_fmaf(s[kvs][r], c2, -m2c));
          rowsum += s[kvs][r];
        }
      {
        float lo, hi2;
        ba_half_pair(rowsum, lo, hi2);
        lsum += (lo + hi2) * (1.f / BA_FP8_PSCALE);
      }
      // P -> e4m3, in accumulator order: byte 16 kvs + r of the B operand
      i32x8_t pb;
#pragma unroll
      for (int kvs = 0; kvs < 2; ++kvs)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          pb[4 * kvs + g] =
              ba_fp8_pack4(s[kvs][4 * g], s[kvs][4 * g + 1], s[kvs][4 * g + 2],
                           s[kvs][4 * g + 3]);
      // O^T += mfma(V^T, P^T): lane's v channel 32 dt + l31, the tile's 64
      // kv rows in one instruction
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt)
        ot[dt] = ba_fp8_mma(ba_fp8_ld_vt(ldsVT(cur), dt * 32 + l31, 2 * hi),
                            pb, ot[dt]);
    }
    if (has_next) write_lds(cur ^ 1, kreg, vreg);
    __syncthreads();
    cur ^= 1;
    if constexpr (HAS_SC) dk_cur = dk_next;
  }

  // scaled form: the 128 store multipliers dv[d] / c take the LDS slot the
  // carry-in multipliers had (read before the loop's first barrier; the
  // loop's last barrier is behind every wave here)
  const float* outm = (const float*)(lds + 2 * 2 * TILEB);
  if constexpr (HAS_SC) {
    if (tid < D)
      ((float*)(lds + 2 * 2 * TILEB))[tid] =
          dvp[tid] * (1.f / BA_FP8_PSCALE);
    __syncthreads();
  }

  if (q_row < Sq) {
    if (OUT_STATE) {
      float* arow = st_acc + b * a_sb + (int64_t)q_row * a_ss + n * a_sh;
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if constexpr (HAS_SC)
            arow[dt * 32 + ba_crow(r, hi)] =
                ot[dt][r] * outm[dt * 32 + ba_crow(r, hi)];
          else
            arow[dt * 32 + ba_crow(r, hi)] = ot[dt][r] * x.out_mul;
      if (hi == 0) {
        st_m[b * ml_sb + n * ml_sh + q_row] = m2;
        st_l[b * ml_sb + n * ml_sh + q_row] = lsum;
      }
    } else {
      // scaled form: dv[d] / c is per channel, 1 / l per row
      const float inv_l = (HAS_SC ? 1.f : x.out_mul) / lsum;
      float* orow = o + (((int64_t)b * Sq + q_row) * N + n) * D;
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if constexpr (HAS_SC)
            orow[dt * 32 + ba_crow(r, hi)] =
                ot[dt][r] * outm[dt * 32 + ba_crow(r, hi)] * inv_l;
          else
            orow[dt * 32 + ba_crow(r, hi)] = ot[dt][r] * inv_l;
      if (hi == 0)
        lse[((int64_t)b * N + n) * Sq + q_row] = BA_LN2 * (m2 + log2f(lsum));
    }
  }
}

template <int OUT_STATE, typename... SC>
void launch_fp8_fwd(const fwd_args& a, const fp8_extra& x, int64_t B,
                    hipStream_t stream, SC... sc) {
  const dim3 grid((unsigned)((a.Sq + BA_FP8_BLOCK - 1) / BA_FP8_BLOCK),
                  (unsigned)a.N, (unsigned)B);
  attn_fp8_fwd_kernel<OUT_STATE, SC...><<<grid, dim3(BA_FP8_NT), 0, stream>>>(
      (const char*)a.q, (const char*)a.k, a.o, a.lse, a.Sq, a.Sk, a.N, a.G,
      a.q_sb, a.q_ss, a.q_sh, a.k_sb, a.k_ss, a.k_sh, a.causal, a.st_acc,
      a.st_m, a.st_l, a.a_sb, a.a_ss, a.a_sh, a.ml_sb, a.ml_sh, a.carry_in, x,
      sc...);
}

bool fp8_descale_ok(float d) { return __builtin_isfinite(d) && d > 0.f; }

// The FP8 forward: the checks of the plain call and its own, the V^T image
// pre-pass, then the one kernel.  Every refusal comes before any launch.
// `sa` non-null is the block-scaled call: the three floats are then ones.
int fp8_fwd_entry(const ba_fp8_scale_args* sa, int out_state, const void* q,
                  const void* k, const void* v, float* o, float* lse, int64_t B, int64_t Sq, int64_t Sk,
                  int64_t N, int64_t Nk, int64_t D, const int64_t* qs,
                  const int64_t* ks, const int64_t* vs, float scale,
                  int causal, int dtype, float* acc, float* m, float* l,
                  const int64_t* as, const int64_t* mls, int carry_in,
                  float dq, float dk, float dv, void* ws, int64_t ws_bytes,
                  void* stream) {
  if (dtype != BAHIP_F8E4M3)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "fp8 forward: unsupported dtype %d (BAHIP_F8E4M3 only)",
                   dtype);
  if (D != BA_FP8_D)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "fp8 forward: unsupported head_dim %d (128 only)", (int)D);
  if (causal && Sq != Sk)
    return ba_fail(BAHIP_ERR_CAUSAL_SHAPE,
                   "causal tiles require Sq == Sk (%d vs %d)", (int)Sq,
                   (int)Sk);
  const int64_t G = ba_gqa_group(N, Nk);
  if (!G)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "q heads N=%d must be a positive multiple of kv heads "
                   "Nk=%d",
                   (int)N, (int)Nk);
  if (sa && (!sa->dq || !sa->dk || !sa->dv || sa->k_tile0 < 0))
    return ba_fail(BAHIP_ERR_DESCALE,
                   "fp8 scaled forward: descale tensors (%p, %p, %p) must "
                   "all be given and k_tile0 = %d must not be negative",
                   (const void*)sa->dq, (const void*)sa->dk,
                   (const void*)sa->dv, sa->k_tile0);
  if (!fp8_descale_ok(dq) || !fp8_descale_ok(dk) || !fp8_descale_ok(dv))
    return ba_fail(BAHIP_ERR_DESCALE,
                   "fp8 descale (%g, %g, %g): every entry must be positive "
                   "and finite",
                   (double)dq, (double)dk, (double)dv);
  ba_fwd_knobs kn;
  kn.vpath = ba_env_int(BA_FWD_KNOB_SPECS[0].env, kn.vpath);
  kn.subt = ba_env_int(BA_FWD_KNOB_SPECS[1].env, kn.subt);
  kn.nt = ba_env_int(BA_FWD_KNOB_SPECS[2].env, kn.nt);
  kn.nbuf = ba_env_int(BA_FWD_KNOB_SPECS[3].env, kn.nbuf);
  kn.kreg = ba_env_int(BA_FWD_KNOB_SPECS[4].env, kn.kreg);
  const ba_fwd_choice c = ba_fwd_select(kn);
  if (c.bad_knob)
    return ba_fail(BAHIP_ERR_BAD_KNOB, "%s=%d is not an accepted value",
                   c.bad_knob, c.bad_value);
  const ba_seg_verdict sv = ba_seg_fwd_support(kn);
  if (sv.knob)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "%s=%d does not support fp8 (default forward variant only)",
                   sv.knob, sv.value);
  if (B < 1 || B > 65535 || N > 65535 || Sq < 1 || Sk < 1 ||
      Sq > INT32_MAX / 2 || Sk > INT32_MAX / 2)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "fp8 forward: unsupported shape B=%d Sq=%lld Sk=%lld N=%d",
                   (int)B, (long long)Sq, (long long)Sk, (int)N);
  const int64_t* strides[3] = {qs, ks, vs};
  const void* bases[3] = {q, k, v};
  static const char* const tname[3] = {"q", "k", "v"};
  static const char* const sname[3] = {"batch", "seq", "head"};
  for (int i = 0; i < 3; ++i) {
    if ((uintptr_t)bases[i] % 16)
      return ba_fail(BAHIP_ERR_UNSUPPORTED,
                     "fp8 forward: %s base pointer %p is not 16-byte aligned",
                     tname[i], bases[i]);
    for (int j = 0; j < 3; ++j)
      if (strides[i][j] % 16)
        return ba_fail(BAHIP_ERR_UNSUPPORTED,
                       "fp8 forward: %s %s stride %lld is not a multiple of "
                       "16 elements (16-byte rows)",
                       tname[i], sname[j], (long long)strides[i][j]);
  }
  const int64_t need = ba_fp8_ws_bytes(B, Sk, Nk);
  if (!ws || ws_bytes < need)
    return ba_fail(BAHIP_ERR_WORKSPACE,
                   "fp8 V^T image workspace of %lld bytes is smaller than "
                   "the %lld needed",
                   (long long)(ws ? ws_bytes : 0), (long long)need);
  static const int64_t none[3] = {0, 0, 0};
  if (!out_state) as = mls = none;
  const fwd_args a = {q, k, v, o, lse, (int)Sq, (int)Sk, (int)N, (int)G,
                      qs[0], qs[1], qs[2], ks[0], ks[1], ks[2],
                      vs[0], vs[1], vs[2], scale, causal, acc, m, l,
                      as[0], as[1], as[2], mls[0], mls[1], carry_in};
  const fp8_extra x = {
      (const char*)ws,
      (float)((double)scale * dq * dk * 1.44269504088896340736),
      BA_FP8_PSCALE / dv, dv / BA_FP8_PSCALE};
  if (!(x.c2 > 0.f) || !__builtin_isfinite(x.c2))
    return ba_fail(BAHIP_ERR_DESCALE,
                   "fp8 forward: descale_q * descale_k * softmax_scale = %g "
                   "must be positive and finite",
                   (double)scale * dq * dk);
  // a finite descale_v can still be small or large enough that one of its
  // multipliers is not: 0 * inf on an empty carry-in acc would be a NaN
  if (!fp8_descale_ok(x.in_mul) || !fp8_descale_ok(x.out_mul))
    return ba_fail(BAHIP_ERR_DESCALE,
                   "fp8 forward: descale_v = %g leaves the multipliers %g / "
                   "descale_v or descale_v / %g outside the positive finite "
                   "floats",
                   (double)dv, (double)BA_FP8_PSCALE, (double)BA_FP8_PSCALE);
  attn_fp8_vt_kernel<<<dim3((unsigned)ba_fp8_tiles(Sk), (unsigned)Nk,
                            (unsigned)B),
                       dim3(BA_FP8_NT), 0, (hipStream_t)stream>>>(
      (const char*)v, (char*)ws, (int)Sk, (int)Nk, vs[0], vs[1], vs[2]);
  BA_CHECK_LAUNCH();
  if (sa) {
    if (out_state)
      launch_fp8_fwd<1>(a, x, B, (hipStream_t)stream, *sa);
    else
      launch_fp8_fwd<0>(a, x, B, (hipStream_t)stream, *sa);
  } else if (out_state) {
    launch_fp8_fwd<1>(a, x, B, (hipStream_t)stream);
  } else {
    launch_fp8_fwd<0>(a, x, B, (hipStream_t)stream);
  }
  return ba_launch_status();
}

}  // namespace

extern "C" int64_t bahip_attn_fwd_f8_workspace_bytes(int64_t B, int64_t Sk,
                                                      int64_t Nk, int64_t D) {
  return D == BA_FP8_D ? ba_fp8_ws_bytes(B, Sk, Nk) : 0;
}

extern "C" int bahip_attn_fwd_f8(
    const void* q, const void* k, const void* v, float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float descale_q, float descale_k, float descale_v, void* workspace,
    int64_t workspace_bytes, void* stream) {
  return fp8_fwd_entry(nullptr, 0, q, k, v, o, lse, B, Sq, Sk, N, Nk, D, q_strides,
                       k_strides, v_strides, softmax_scale, causal, dtype,
                       nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                       descale_q, descale_k, descale_v, workspace,
                       workspace_bytes, stream);
}

extern "C" int bahip_attn_fwd_accum_f8(
    void* hip_function, const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in, float descale_q,
    float descale_k, float descale_v, void* workspace,
    int64_t workspace_bytes, void* stream) {
  if (hip_function)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "fp8 does not support a module-launched forward");
  return fp8_fwd_entry(nullptr, 1, q, k, v, nullptr, nullptr, B, Sq, Sk, N, Nk, D,
                       q_strides, k_strides, v_strides, softmax_scale, causal,
                       dtype, acc, m, l, acc_strides, ml_strides, carry_in,
                       descale_q, descale_k, descale_v, workspace,
                       workspace_bytes, stream);
}

// ---- block-scaled entry points ---------------------------------------------
namespace {
ba_fp8_scale_args fp8_scale_args(const float* dq, const float* dk,
                                 const float* dv, const int64_t* dqs,
                                 const int64_t* dks, const int64_t* dvs,
                                 int64_t k_tile0) {
  static const int64_t none[2] = {0, 0};
  if (!dqs || !dks || !dvs) dq = nullptr, dqs = dks = dvs = none;
  const bool tile_ok = k_tile0 >= 0 && k_tile0 <= INT32_MAX / 2;
  return {dq, dk, dv, dqs[0], dqs[1], dks[0], dks[1], dvs[0], dvs[1],
          tile_ok ? (int)k_tile0 : -1};
}
}  // namespace

extern "C" int bahip_attn_fwd_f8_scaled(
    const void* q, const void* k, const void* v, float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    const float* descale_q, const float* descale_k, const float* descale_v,
    const int64_t dq_strides[2], const int64_t dk_strides[2],
    const int64_t dv_strides[2], int64_t k_tile0, void* workspace,
    int64_t workspace_bytes, void* stream) {
  const ba_fp8_scale_args sa =
      fp8_scale_args(descale_q, descale_k, descale_v, dq_strides, dk_strides,
                     dv_strides, k_tile0);
  return fp8_fwd_entry(&sa, 0, q, k, v, o, lse, B, Sq, Sk, N, Nk, D, q_strides,
                       k_strides, v_strides, softmax_scale, causal, dtype,
                       nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1.f,
                       1.f, 1.f, workspace, workspace_bytes, stream);
}

extern "C" int bahip_attn_fwd_accum_f8_scaled(
    void* hip_function, const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in, const float* descale_q,
    const float* descale_k, const float* descale_v,
    const int64_t dq_strides[2], const int64_t dk_strides[2],
    const int64_t dv_strides[2], int64_t k_tile0, void* workspace,
    int64_t workspace_bytes, void* stream) {
  if (hip_function)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "fp8 does not support a module-launched forward");
  const ba_fp8_scale_args sa =
      fp8_scale_args(descale_q, descale_k, descale_v, dq_strides, dk_strides,
                     dv_strides, k_tile0);
  return fp8_fwd_entry(&sa, 1, q, k, v, nullptr, nullptr, B, Sq, Sk, N, Nk, D,
                       q_strides, k_strides, v_strides, softmax_scale, causal,
                       dtype, acc, m, l, acc_strides, ml_strides, carry_in,
                       1.f, 1.f, 1.f, workspace, workspace_bytes, stream);
}
