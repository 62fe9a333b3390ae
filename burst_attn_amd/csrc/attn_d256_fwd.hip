// head_dim 256 forward tile kernel for gfx950 (design: attn_d256.h).
//
//   * workgroup = 4 waves (256 threads), one per SIMD; wave w owns q rows
//     [blk*128 + w*32, +32); grid = (ceil(Sq/128), N, B).
//   * 64-row kv tiles in LDS, double buffered, one barrier per tile; the
//     next tile's global loads are issued before the current tile's MFMAs.
//     K is row-major [kv][256] (512-byte rows, 16-byte XOR swizzle over the
//     whole row); V is transposed at staging time into [256][kv] (128-byte
//     rows, the D = 128 kernel's V^T image with four times the rows).
//     2 x (32 + 32) KiB = 128 KiB: one workgroup per CU.
//   * per 32-kv subtile and wave: S^T = mfma(K, Q) (16 MFMAs, each K
//     fragment read from LDS right before its MFMA), lane-local online
//     softmax in the exp2 domain with defer-max, P -> fragments in
//     registers, O^T += mfma(V^T, P^T) (16 MFMAs).
//   * resident per lane: the O^T accumulator (8 x 16 fp32) and the Q
//     fragments (16 x 4 dwords); 16 staging dwordx4 in flight.
//   * OUT_STATE as in attn_fwd.hip: 0 = normalised o + lse, 1 = the
//     carry-in / carry-out state (acc, m, l), bit-compatible with the
//     D = 64/128 kernels' so state init, finalize and the ring's merge are
//     shared.
//   * CAP: empty = the plain kernel.  One ba_cap_args = the soft-capped form
//     (attn_common.h), by the rules of attn_fwd.hip's: the row max on raw
//     scores with only that one value transformed, t = tanh(.) per score,
//     p = exp2(t * c2cap - m2), and the mask applied to t.

#include "attn_d256.h"

namespace {

template <typename T, int OUT_STATE, typename... CAP>
__global__ __launch_bounds__(BA_D256_NT) void attn_d256_fwd_kernel(
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
    int64_t ml_sb, int64_t ml_sh, int carry_in, CAP... cap) {
  using MT = mfma_traits<T>;
  using frag = typename MT::frag;
  constexpr bool HAS_CAP = ba_pack_is<ba_cap_args, CAP...>;
  static_assert(HAS_CAP || sizeof...(CAP) == 0, "the pack: one ba_cap_args");
  constexpr int D = BA_D256;
  constexpr int NT = BA_D256_NT;
  constexpr int KVBLK = 64;
  // K image rows are 512 bytes; 16 slots of 16 bytes already span all 64
  // banks, so the D = 128 swizzle serves (and leaves bit 8 of a row offset
  // to plain addition, see stage_rc)
  constexpr int SWZ_K = 15;
  constexpr int SWZ_V = 7;   // V^T image rows are 128 bytes
  constexpr int PT = (KVBLK * D / 8) / NT;  // 8 chunks per thread and image

  // one LDS object: [2 buffers][K row-major | V transposed][KVBLK * D]
  __shared__ T lds[2 * 2 * KVBLK * D];
  auto ldsK = [&](int buf) -> T* { return lds + buf * (2 * KVBLK * D); };
  auto ldsVT = [&](int buf) -> T* {
    return lds + buf * (2 * KVBLK * D) + KVBLK * D;
  };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31;
  const int hi = lane >> 5;
  const int n = blockIdx.y;
  const int b = blockIdx.z;
  const int qb = blockIdx.x * BA_D256_BLOCK + wave * 32;
  const int q_row = qb + l31;

  const T* qp = q + (int64_t)b * q_sb + (int64_t)n * q_sh;
  const int nkv = n / G;  // grouped-query heads: q head n attends n / G
  const T* kp = k + (int64_t)b * k_sb + (int64_t)nkv * k_sh;
  const T* vp = v + (int64_t)b * v_sb + (int64_t)nkv * v_sh;

  // Q fragments: B operand of S^T = mfma(K, Q); lane holds q row q_row,
  // elements d = 16 s + 8 hi + j
  frag qf[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    u32x4_t w = {0, 0, 0, 0};
    if (q_row < Sq)
      w = *(const u32x4_t*)(qp + (int64_t)q_row * q_ss + 16 * s + 8 * hi);
    qf[s] = __builtin_bit_cast(frag, w);
  }

  const float c2 = scale * BA_LOG2E;  // exp2-domain scale
  ba_cap_args cp = {0.f, 0.f};
  if constexpr (HAS_CAP) cp = ba_cap_of(cap...);
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
      for (int r = 0; r < 16; ++r) ot[dt][r] = arow[dt * 32 + ba_crow(r, hi)];
  }

  // causal: no key past the block's last row is visible to any of its rows
  const int kv_limit =
      causal ? min(Sk, (int)(blockIdx.x + 1) * BA_D256_BLOCK) : Sk;
  const int nt = (kv_limit + KVBLK - 1) / KVBLK;

  // (row, 8-element column) of this thread's chunk c of a staged tile.
  // Eight consecutive threads cover 128 contiguous bytes of a row; c steps
  // the column by 64 elements (c & 3) and the row by 32 (c >> 2).  Both
  // steps leave every swizzle term of the K and V^T images unchanged, so a
  // thread's 8 + 64 LDS write addresses differ by constants and one XOR:
  // with the D = 128 kernels' thread-major chunk order each address needs a
  // register of its own, which is what spilled here.
  auto stage_rc = [&](int c) {
    struct rc {
      int row, col8;
    };
    return rc{(tid >> 3) + 32 * (c >> 2), (tid & 7) + 8 * (c & 3)};
  };
  auto issue_loads = [&](int tile, u32x4_t* kreg, u32x4_t* vreg) {
    const int kv0 = tile * KVBLK;
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      const auto [row, col8] = stage_rc(c);
      // clamped, not guarded (see attn_fwd.hip): rows past Sk re-load row
      // Sk - 1 and the kv-range mask gives them p = 0
      const int kvg = kv0 + row;
      const int kvc = kvg < Sk ? kvg : (Sk - 1);
      kreg[c] = *(const u32x4_t*)(kp + (int64_t)kvc * k_ss + col8 * 8);
      vreg[c] = *(const u32x4_t*)(vp + (int64_t)kvc * v_ss + col8 * 8);
    }
  };
  auto write_lds = [&](int buf, const u32x4_t* kreg, const u32x4_t* vreg) {
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      const auto [row, col8] = stage_rc(c);
      const int byte = ba_swz<SWZ_K>(row * (2 * D) + col8 * 16, row);
      *(u32x4_t*)((char*)ldsK(buf) + byte) = kreg[c];
      ba_st_transposed<T, KVBLK, SWZ_V, 7>(ldsVT(buf), row, col8 * 8, vreg[c]);
    }
  };

  {
    u32x4_t kreg[PT], vreg[PT];
    issue_loads(0, kreg, vreg);
    write_lds(0, kreg, vreg);
    __syncthreads();
  }

  constexpr float DEFER_THR = 8.f;  // defer-max threshold, exp2 domain
  int cur = 0;
  for (int t = 0; t < nt; ++t) {
    const int kv0 = t * KVBLK;
    const bool has_next = (t + 1) < nt;
    u32x4_t kreg[PT], vreg[PT];
    if (has_next) issue_loads(t + 1, kreg, vreg);

    // causal: a tile wholly above the diagonal of this wave's 32 rows
    if (!causal || kv0 <= qb + 31) {
      // a full tile needs no mask: inside Sk and, if causal, at or below
      // the diagonal for every row of this wave
      const bool full =
          (kv0 + KVBLK <= Sk) && (!causal || (kv0 + KVBLK - 1 <= qb));
#pragma unroll
      for (int kvs = 0; kvs < 2; ++kvs) {
        // S^T = mfma(K, Q): raw, unscaled scores
        f32x16_t s = (f32x16_t)(0.f);
#pragma unroll
        for (int i = 0; i < D / 16; ++i)
          s = MT::mma(ba_ld_rowslice<T, D, SWZ_K>(ldsK(cur), kvs * 32 + l31,
                                                  16 * i + 8 * hi),
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
          // cap form: the capped value of the one max (tanh is increasing)
          if constexpr (HAS_CAP)
            tm = ba_cap_tanh(fmaxf(lo, hi2), cp.a) * cp.c2;
          else
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
          for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[dt][r] *= alpha;
        }
        float rowsum = 0.f;
        if constexpr (HAS_CAP) {
          // m2 is a capped level (>= -c2cap) by now.  A masked entry is
          // masked on t: tanh of the raw mask level is -1, a finite score
          // of -softcap that would leak
          if (!full) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float t = ba_cap_tanh(s[r], cp.a);
              s[r] = ba_exp2(__builtin_fmaf(
                  s[r] == BA_NEG_BIG ? BA_NEG_BIG : t, cp.c2, -m2));
              rowsum += s[r];
            }
          } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              s[r] =
                  ba_exp2(__builtin_fmaf(ba_cap_tanh(s[r], cp.a), cp.c2, -m2));
              rowsum += s[r];
            }
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            s[r] = ba_exp2(__builtin_fmaf(s[r], c2, -m2));
            rowsum += s[r];
          }
        }
        {
          float lo, hi2;
          ba_half_pair(rowsum, lo, hi2);
          lsum += lo + hi2;
        }
        frag pf[2];
        ba_build_frag_pair<T>(s, pf);
        // O^T += mfma(V^T, P^T): lane's d row 32 dt + l31, kv columns
        // [32 kvs + 16 u, +16)
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt)
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
      for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          arow[dt * 32 + ba_crow(r, hi)] = ot[dt][r];
      if (hi == 0) {
        st_m[b * ml_sb + n * ml_sh + q_row] = m2;
        st_l[b * ml_sb + n * ml_sh + q_row] = lsum;
      }
    } else {
      const float inv_l = 1.f / lsum;
      float* orow = o + (((int64_t)b * Sq + q_row) * N + n) * D;
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          orow[dt * 32 + ba_crow(r, hi)] = ot[dt][r] * inv_l;
      if (hi == 0)
        lse[((int64_t)b * N + n) * Sq + q_row] = BA_LN2 * (m2 + log2f(lsum));
    }
  }
}

// `cap`: nothing, or the ba_cap_args of the soft-capped kernel
template <typename T, int OUT_STATE, typename... CAP>
void launch_d256_fwd(const fwd_args& a, int64_t B, hipStream_t stream,
                     CAP... cap) {
  const dim3 grid((unsigned)((a.Sq + BA_D256_BLOCK - 1) / BA_D256_BLOCK),
                  (unsigned)a.N, (unsigned)B);
  attn_d256_fwd_kernel<T, OUT_STATE, CAP...>
      <<<grid, dim3(BA_D256_NT), 0, stream>>>(
      (const T*)a.q, (const T*)a.k, (const T*)a.v, a.o, a.lse, a.Sq, a.Sk,
      a.N, a.G, a.q_sb, a.q_ss, a.q_sh, a.k_sb, a.k_ss, a.k_sh, a.v_sb, a.v_ss,
      a.v_sh, a.scale, a.causal, a.st_acc, a.st_m, a.st_l, a.a_sb, a.a_ss,
      a.a_sh, a.ml_sb, a.ml_sh, a.carry_in, cap...);
}

}  // namespace

int ba_d256_fwd(const fwd_args& a, int out_state, int64_t B, int dtype,
                hipStream_t stream) {
  return ba_dispatch_t256(dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    if (out_state)
      launch_d256_fwd<T, 1>(a, B, stream);
    else
      launch_d256_fwd<T, 0>(a, B, stream);
    return ba_launch_status();
  });
}

int ba_d256_fwd_cap(const fwd_args& a, const ba_cap_args& cp, int out_state,
                    int64_t B, int dtype, hipStream_t stream) {
  return ba_dispatch_t256(dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    if (out_state)
      launch_d256_fwd<T, 1>(a, B, stream, cp);
    else
      launch_d256_fwd<T, 0>(a, B, stream, cp);
    return ba_launch_status();
  });
}
