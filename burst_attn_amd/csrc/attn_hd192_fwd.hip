// qk head_dim 192 / v head_dim 128 forward tile kernel for gfx950 (design:
// attn_hd192.h), and the forward entry points that take both widths.
//
//   * workgroup = 4 waves (256 threads), one per SIMD; wave w owns q rows
//     [blk*128 + w*32, +32); grid = (ceil(Sq/128), N, B).
//   * 64-row kv tiles in LDS, double buffered, one barrier per tile; the
//     next tile's global loads are issued before the current tile's MFMAs.
//     K is row-major [kv][192] in padded 400-byte rows, unswizzled
//     (attn_hd192.h); V is transposed at staging time into [128][kv]
//     (128-byte rows, the D = 128 kernel's V^T image).
//     2 x (25 + 16) KiB = 82 KiB: one workgroup per CU.
//   * per 32-kv subtile and wave: S^T = mfma(K, Q) over 192 (12 MFMAs, each
//     K fragment read from LDS right before its MFMA), lane-local online
//     softmax in the exp2 domain with defer-max, P -> fragments in
//     registers, O^T += mfma(V^T, P^T) over the subtile into 128 rows (8
//     MFMAs).
//   * resident per lane: the O^T accumulator (4 x 16 fp32) and the Q
//     fragments (12 x 4 dwords); 6 + 4 staging dwordx4 in flight.
//   * OUT_STATE as in attn_fwd.hip: 0 = normalised o + lse, 1 = the
//     carry-in / carry-out state (acc, m, l), 128 wide and bit-compatible
//     with the D = 128 kernels' so state init and finalize are theirs.

#include "attn_hd192.h"
#include "fwd_variants.h"
#include "gqa_heads.h"
#include "bwd_plans.h"
#include "seg_support.h"

namespace {

template <typename T, int OUT_STATE>
__global__ __launch_bounds__(BA_HD192_NT) void attn_hd192_fwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
    float* __restrict__ o, float* __restrict__ lse,
    int Sq, int Sk, int N, int G,
    int64_t q_sb, int64_t q_ss, int64_t q_sh,
    int64_t k_sb, int64_t k_ss, int64_t k_sh,
    int64_t v_sb, int64_t v_ss, int64_t v_sh,
    float scale, int causal,
    float* __restrict__ st_acc, float* __restrict__ st_m,
    float* __restrict__ st_l,
    int64_t a_sb, int64_t a_ss, int64_t a_sh,
    int64_t ml_sb, int64_t ml_sh, int carry_in) {
  using MT = mfma_traits<T>;
  using frag = typename MT::frag;
  constexpr int DQK = BA_HD192_DQK;
  constexpr int DV = BA_HD192_DV;
  constexpr int NT = BA_HD192_NT;
  constexpr int KVBLK = 64;
  constexpr int SWZ_V = 7;  // V^T image rows are 128 bytes
  constexpr int PTK = (KVBLK * DQK / 8) / NT;  // 6 K chunks per thread
  constexpr int PTV = (KVBLK * DV / 8) / NT;   // 4 V chunks per thread
  constexpr int KBYTES = KVBLK * BA_HD192_ROWB;
  constexpr int BUFBYTES = KBYTES + DV * KVBLK * (int)sizeof(T);

  // one LDS object: [2 buffers][K row-major, padded rows | V transposed]
  __shared__ __attribute__((aligned(16))) char lds[2 * BUFBYTES];
  auto ldsK = [&](int buf) -> char* { return lds + buf * BUFBYTES; };
  auto ldsVT = [&](int buf) -> T* {
    return (T*)(lds + buf * BUFBYTES + KBYTES);
  };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31;
  const int hi = lane >> 5;
  const int n = blockIdx.y;
  const int b = blockIdx.z;
  const int qb = blockIdx.x * BA_HD192_BLOCK + wave * 32;
  const int q_row = qb + l31;

  const T* qp = q + (int64_t)b * q_sb + (int64_t)n * q_sh;
  const int nkv = n / G;  // grouped-query heads: q head n attends n / G
  const T* kp = k + (int64_t)b * k_sb + (int64_t)nkv * k_sh;
  const T* vp = v + (int64_t)b * v_sb + (int64_t)nkv * v_sh;

  // Q fragments: B operand of S^T = mfma(K, Q); lane holds q row q_row,
  // elements d = 16 s + 8 hi + j
  frag qf[DQK / 16];
#pragma unroll
  for (int s = 0; s < DQK / 16; ++s) {
    u32x4_t w = {0, 0, 0, 0};
    if (q_row < Sq)
      w = *(const u32x4_t*)(qp + (int64_t)q_row * q_ss + 16 * s + 8 * hi);
    qf[s] = __builtin_bit_cast(frag, w);
  }

  const float c2 = scale * BA_LOG2E;  // exp2-domain scale
  float m2 = BA_NEG_BIG;
  float lsum = 0.f;
  f32x16_t ot[DV / 32];
#pragma unroll
  for (int dt = 0; dt < DV / 32; ++dt) ot[dt] = (f32x16_t)(0.f);
  if (OUT_STATE && carry_in && q_row < Sq) {
    m2 = st_m[b * ml_sb + n * ml_sh + q_row];
    lsum = st_l[b * ml_sb + n * ml_sh + q_row];
    const float* arow = st_acc + b * a_sb + (int64_t)q_row * a_ss + n * a_sh;
#pragma unroll
    for (int dt = 0; dt < DV / 32; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) ot[dt][r] = arow[dt * 32 + ba_crow(r, hi)];
  }

  // causal: no key past the block's last row is visible to any of its rows
  const int kv_limit =
      causal ? min(Sk, (int)(blockIdx.x + 1) * BA_HD192_BLOCK) : Sk;
  const int nt = (kv_limit + KVBLK - 1) / KVBLK;

  auto issue_loads = [&](int tile, u32x4_t* kreg, u32x4_t* vreg) {
    const int kv0 = tile * KVBLK;
    // clamped, not guarded (see attn_fwd.hip): rows past Sk re-load row
    // Sk - 1 and the kv-range mask gives them p = 0
#pragma unroll
    for (int c = 0; c < PTK; ++c) {
      const auto [row, col8] = ba_hd192_rc_qk(c);
      const int kvg = kv0 + row;
      const int kvc = kvg < Sk ? kvg : (Sk - 1);
      kreg[c] = *(const u32x4_t*)(kp + (int64_t)kvc * k_ss + col8 * 8);
    }
#pragma unroll
    for (int c = 0; c < PTV; ++c) {
      const auto [row, col8] = ba_hd192_rc_v(c);
      const int kvg = kv0 + row;
      const int kvc = kvg < Sk ? kvg : (Sk - 1);
      vreg[c] = *(const u32x4_t*)(vp + (int64_t)kvc * v_ss + col8 * 8);
    }
  };
  auto write_lds = [&](int buf, const u32x4_t* kreg, const u32x4_t* vreg) {
#pragma unroll
    for (int c = 0; c < PTK; ++c) {
      const auto [row, col8] = ba_hd192_rc_qk(c);
      ba_st_row192(ldsK(buf), row, col8, kreg[c]);
    }
#pragma unroll
    for (int c = 0; c < PTV; ++c) {
      const auto [row, col8] = ba_hd192_rc_v(c);
      ba_st_transposed<T, KVBLK, SWZ_V, 7>(ldsVT(buf), row, col8 * 8, vreg[c]);
    }
  };

  {
    u32x4_t kreg[PTK], vreg[PTV];
    issue_loads(0, kreg, vreg);
    write_lds(0, kreg, vreg);
    __syncthreads();
  }

  constexpr float DEFER_THR = 8.f;  // defer-max threshold, exp2 domain
  int cur = 0;
  for (int t = 0; t < nt; ++t) {
    const int kv0 = t * KVBLK;
    const bool has_next = (t + 1) < nt;
    u32x4_t kreg[PTK], vreg[PTV];
    if (has_next) issue_loads(t + 1, kreg, vreg);

    // causal: a tile wholly above the diagonal of this wave's 32 rows
    if (!causal || kv0 <= qb + 31) {
      // a full tile needs no mask: inside Sk and, if causal, at or below
      // the diagonal for every row of this wave
      const bool full =
          (kv0 + KVBLK <= Sk) && (!causal || (kv0 + KVBLK - 1 <= qb));
#pragma unroll
      for (int kvs = 0; kvs < 2; ++kvs) {
        // S^T = mfma(K, Q) over the 192 q/k channels: raw, unscaled scores
        f32x16_t s = (f32x16_t)(0.f);
#pragma unroll
        for (int i = 0; i < DQK / 16; ++i)
          s = MT::mma(
              ba_ld_row192<T>(ldsK(cur), kvs * 32 + l31, 16 * i + 8 * hi),
              qf[i], s);
        if (!full) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kv_g = kv0 + kvs * 32 + ba_crow(r, 0) + 4 * hi;
            if (!(kv_g < Sk && (!causal || kv_g <= q_row))) s[r] = BA_NEG_BIG;
          }
        }
        // row max on raw scores (max commutes with c2 > 0)
        float tm = ba_max16(s);
        {
          float lo, hi2;
          ba_half_pair(tm, lo, hi2);
          tm = fmaxf(lo, hi2) * c2;
        }
        // defer-max: skip the O/l rescale while the running max grows by
        // <= THR; decided before these scores are exponentiated
        if (!__all(tm - m2 <= DEFER_THR)) {
          const float mnew = fmaxf(m2, tm);
          const float alpha = ba_exp2(m2 - mnew);
          m2 = mnew;
          lsum *= alpha;
#pragma unroll
          for (int dt = 0; dt < DV / 32; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[dt][r] *= alpha;
        }
        float rowsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s[r] = ba_exp2(__builtin_fmaf(s[r], c2, -m2));
          rowsum += s[r];
        }
        {
          float lo, hi2;
          ba_half_pair(rowsum, lo, hi2);
          lsum += lo + hi2;
        }
        frag pf[2];
        ba_build_frag_pair<T>(s, pf);
        // O^T += mfma(V^T, P^T): lane's v channel 32 dt + l31, kv columns
        // [32 kvs + 16 u, +16)
#pragma unroll
        for (int dt = 0; dt < DV / 32; ++dt)
#pragma unroll
          for (int u = 0; u < 2; ++u)
            ot[dt] = MT::mma(
                ba_ld_rowslice<T, KVBLK, SWZ_V, 7>(
                    ldsVT(cur), dt * 32 + l31, kvs * 32 + 16 * u + 8 * hi),
                pf[u], ot[dt]);
      }
    }
    if (has_next) write_lds(cur ^ 1, kreg, vreg);
    __syncthreads();
    cur ^= 1;
  }

  if (q_row < Sq) {
    if (OUT_STATE) {
      float* arow = st_acc + b * a_sb + (int64_t)q_row * a_ss + n * a_sh;
#pragma unroll
      for (int dt = 0; dt < DV / 32; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          arow[dt * 32 + ba_crow(r, hi)] = ot[dt][r];
      if (hi == 0) {
        st_m[b * ml_sb + n * ml_sh + q_row] = m2;
        st_l[b * ml_sb + n * ml_sh + q_row] = lsum;
      }
    } else {
      const float inv_l = 1.f / lsum;
      float* orow = o + (((int64_t)b * Sq + q_row) * N + n) * DV;
#pragma unroll
      for (int dt = 0; dt < DV / 32; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          orow[dt * 32 + ba_crow(r, hi)] = ot[dt][r] * inv_l;
      if (hi == 0)
        lse[((int64_t)b * N + n) * Sq + q_row] = BA_LN2 * (m2 + log2f(lsum));
    }
  }
}

template <typename T, int OUT_STATE>
void launch_hd192_fwd(const fwd_args& a, int64_t B, hipStream_t stream) {
  const dim3 grid((unsigned)((a.Sq + BA_HD192_BLOCK - 1) / BA_HD192_BLOCK),
                  (unsigned)a.N, (unsigned)B);
  attn_hd192_fwd_kernel<T, OUT_STATE>
      <<<grid, dim3(BA_HD192_NT), 0, stream>>>(
      (const T*)a.q, (const T*)a.k, (const T*)a.v, a.o, a.lse, a.Sq, a.Sk,
      a.N, a.G, a.q_sb, a.q_ss, a.q_sh, a.k_sb, a.k_ss, a.k_sh, a.v_sb, a.v_ss,
      a.v_sh, a.scale, a.causal, a.st_acc, a.st_m, a.st_l, a.a_sb, a.a_ss,
      a.a_sh, a.ml_sb, a.ml_sh, a.carry_in);
}

// The (192, 128) forward: the checks of the plain call, then the one kernel.
// Only the default BA_FWD_* selection has a form here; every refusal comes
// before the launch.
int hd192_fwd_entry(int out_state, const void* q, const void* k, const void* v,
                    float* o, float* lse, int64_t B, int64_t Sq, int64_t Sk,
                    int64_t N, int64_t Nk, const int64_t* qs,
                    const int64_t* ks, const int64_t* vs, float scale,
                    int causal, int dtype, float* acc, float* m, float* l,
                    const int64_t* as, const int64_t* mls, int carry_in,
                    void* stream) {
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
                   "%s=%d does not support head_dim pair (192, 128) (default "
                   "forward variant only)",
                   sv.knob, sv.value);
  if (B < 1 || B > 65535 || N > 65535 || Sq < 1 || Sk < 1)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "head_dim pair (192, 128): unsupported shape B=%d Sq=%d "
                   "Sk=%d N=%d",
                   (int)B, (int)Sq, (int)Sk, (int)N);
  static const int64_t none[3] = {0, 0, 0};
  if (!out_state) as = mls = none;
  const fwd_args a = {q, k, v, o, lse, (int)Sq, (int)Sk, (int)N, (int)G,
                      qs[0], qs[1], qs[2], ks[0], ks[1], ks[2],
                      vs[0], vs[1], vs[2], scale, causal, acc, m, l,
                      as[0], as[1], as[2], mls[0], mls[1], carry_in};
  return ba_dispatch_t192(dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    if (out_state)
      launch_hd192_fwd<T, 1>(a, B, (hipStream_t)stream);
    else
      launch_hd192_fwd<T, 0>(a, B, (hipStream_t)stream);
    return ba_launch_status();
  });
}

}  // namespace

extern "C" int bahip_attn_fwd_dv(
    const void* q, const void* k, const void* v, float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    int64_t Dv, const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    void* stream) {
  int same;
  if (int rc = ba_hd192_route(D, Dv, &same)) return rc;
  if (same)
    return bahip_attn_fwd_gqa(q, k, v, o, lse, B, Sq, Sk, N, Nk, D, q_strides,
                              k_strides, v_strides, softmax_scale, causal,
                              dtype, stream);
  return hd192_fwd_entry(0, q, k, v, o, lse, B, Sq, Sk, N, Nk, q_strides,
                         k_strides, v_strides, softmax_scale, causal, dtype,
                         nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                         stream);
}

extern "C" int bahip_attn_fwd_accum_dv(
    void* hip_function, const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    int64_t Dv, const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in, void* stream) {
  int same;
  if (int rc = ba_hd192_route(D, Dv, &same)) return rc;
  if (same)
    return bahip_attn_fwd_accum_gqa(hip_function, q, k, v, B, Sq, Sk, N, Nk, D,
                                    q_strides, k_strides, v_strides,
                                    softmax_scale, causal, dtype, acc, m, l,
                                    acc_strides, ml_strides, carry_in, stream);
  if (hip_function)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "head_dim pair (192, 128) does not support a "
                   "module-launched forward");
  return hd192_fwd_entry(1, q, k, v, nullptr, nullptr, B, Sq, Sk, N, Nk,
                         q_strides, k_strides, v_strides, softmax_scale,
                         causal, dtype, acc, m, l, acc_strides, ml_strides,
                         carry_in, stream);
}
