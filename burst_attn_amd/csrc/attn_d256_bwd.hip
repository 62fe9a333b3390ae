// head_dim 256 backward tile kernels for gfx950 (design: attn_d256.h).
//
// The default "split8" plan of attn_bwd.hip at one wave per SIMD: a
// q-resident dq kernel and the kv-resident dV and dK kernels, each adding
// its tile contribution into a strided fp32 accumulator with one
// read-add-write per owned row and no atomics, so the backward is bitwise
// run-to-run deterministic.  Tile math as at the top of attn_bwd.hip:
//     p = exp2(s * c2 - lse * log2e);  dv += p^T do;  dp = do v^T
//     ds = p * (dp - delta) * scale;   dq += ds k;    dk += ds^T q
// Streamed tiles are 32 rows (one MFMA subtile); their transposed images
// have 64-byte rows (ba_swz64, attn_d256.h).
// CAP: empty = the plain kernels.  One ba_cap_args = the soft-capped form
// (attn_common.h): t = tanh(.) recomputed from the raw score,
//     p = exp2(t * c2cap - lse * log2e);  ds = p * (dp - delta) * (1 - t^2) * scale
// with the mask applied to the exponent, never to the raw score.

#include "attn_d256.h"

namespace {

constexpr int D = BA_D256;
constexpr int NT = BA_D256_NT;
constexpr int TILE = 32;                   // streamed rows per tile
constexpr int PT = (TILE * D / 8) / NT;    // 4 chunks per thread and image
// row-major images have 512-byte rows; 16 slots of 16 bytes span all 64
// banks, so the D = 128 swizzle serves
constexpr int SWZ = 15;

// this thread's chunk c of a staged 32 x 256 tile: eight consecutive
// threads cover 128 contiguous bytes of a row, c steps the column by 64
// elements.  That step changes no swizzle term of the row-major or the
// transposed image, so a thread's LDS write addresses of c > 0 are those of
// c = 0 plus a constant (see attn_d256_fwd.hip).
struct chunk_rc {
  int row, col8;
};
__device__ __forceinline__ chunk_rc stage_rc(int c) {
  return {(int)threadIdx.x >> 3, ((int)threadIdx.x & 7) + 8 * c};
}
__device__ __forceinline__ int rowmajor_byte(int row, int col8) {
  return ba_swz<SWZ>(row * (2 * D) + col8 * 16, row);
}

// ====================== dq kernel (q-resident) ==========================
// wave w owns q rows [blk*128 + w*32, +32): Q and dO fragments (64 + 64
// dwords) and the dQ^T accumulator (128) stay in registers; K, V and K^T
// tiles of 32 kv rows stream through LDS, double buffered (96 KiB).
//   S^T = mfma(K, Q); dP^T = mfma(V, dO); dS^T in-lane (lse and delta are
//   lane-local); dQ^T += mfma(K^T, dS^T)
template <typename T, typename... CAP>
__global__ __launch_bounds__(NT) void bwd_d256_dq_kernel(
    const T* __restrict__ dout, const T* __restrict__ q,
    const T* __restrict__ k, const T* __restrict__ v,
    const float* __restrict__ delta, const float* __restrict__ lse,
    float* __restrict__ dq, int Sq, int Sk, int N, int G,
    int64_t g_sb, int64_t g_ss, int64_t g_sh,
    int64_t q_sb, int64_t q_ss, int64_t q_sh,
    int64_t k_sb, int64_t k_ss, int64_t k_sh,
    int64_t v_sb, int64_t v_ss, int64_t v_sh,
    int64_t d_sb, int64_t d_sh, int64_t l_sb, int64_t l_sh,
    int64_t dq_sb, int64_t dq_ss, int64_t dq_sh,
    float scale, int causal, CAP... cap) {
  using MT = mfma_traits<T>;
  using frag = typename MT::frag;
  constexpr bool HAS_CAP = ba_pack_is<ba_cap_args, CAP...>;
  static_assert(HAS_CAP || sizeof...(CAP) == 0, "the pack: one ba_cap_args");
  ba_cap_args cp = {0.f, 0.f};
  if constexpr (HAS_CAP) cp = ba_cap_of(cap...);

  // [2 buffers][K row-major | V row-major | K^T transposed]
  __shared__ T lds[2 * 3 * TILE * D];
  auto ldsK = [&](int buf) -> T* { return lds + buf * (3 * TILE * D); };
  auto ldsV = [&](int buf) -> T* { return lds + buf * (3 * TILE * D) + TILE * D; };
  auto ldsKT = [&](int buf) -> T* {
    return lds + buf * (3 * TILE * D) + 2 * TILE * D;
  };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int n = blockIdx.y, b = blockIdx.z;
  const int qb = blockIdx.x * BA_D256_BLOCK + wave * 32;
  const int q_row = qb + l31;

  const T* qp = q + b * q_sb + (int64_t)n * q_sh;
  const T* gp = dout + b * g_sb + (int64_t)n * g_sh;
  const int nkv = n / G;  // grouped-query heads: q head n reads n / G
  const T* kp = k + b * k_sb + (int64_t)nkv * k_sh;
  const T* vp = v + b * v_sb + (int64_t)nkv * v_sh;

  frag qf[D / 16], gf[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    u32x4_t wq = {0, 0, 0, 0}, wg = {0, 0, 0, 0};
    if (q_row < Sq) {
      wq = *(const u32x4_t*)(qp + (int64_t)q_row * q_ss + 16 * s + 8 * hi);
      wg = *(const u32x4_t*)(gp + (int64_t)q_row * g_ss + 16 * s + 8 * hi);
    }
    qf[s] = __builtin_bit_cast(frag, wq);
    gf[s] = __builtin_bit_cast(frag, wg);
  }
  const float c2 = scale * BA_LOG2E;
  const float lse2 =
      (q_row < Sq) ? lse[b * l_sb + n * l_sh + q_row] * BA_LOG2E : 0.f;
  const float dlt = (q_row < Sq) ? delta[b * d_sb + n * d_sh + q_row] : 0.f;

  f32x16_t dqt[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) dqt[dt] = (f32x16_t)(0.f);

  const int kv_limit =
      causal ? min(Sk, (int)(blockIdx.x + 1) * BA_D256_BLOCK) : Sk;
  const int nt = (kv_limit + TILE - 1) / TILE;

  auto issue_loads = [&](int tile, u32x4_t* kreg, u32x4_t* vreg) {
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      const auto [row, col8] = stage_rc(c);
      // clamped, not guarded: rows past Sk re-load row Sk - 1; their
      // scores are masked to p = 0
      const int kvg = tile * TILE + row;
      const int kvc = kvg < Sk ? kvg : (Sk - 1);
      kreg[c] = *(const u32x4_t*)(kp + (int64_t)kvc * k_ss + col8 * 8);
      vreg[c] = *(const u32x4_t*)(vp + (int64_t)kvc * v_ss + col8 * 8);
    }
  };
  auto write_lds = [&](int buf, const u32x4_t* kreg, const u32x4_t* vreg) {
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      const auto [row, col8] = stage_rc(c);
      const int byte = rowmajor_byte(row, col8);
      *(u32x4_t*)((char*)ldsK(buf) + byte) = kreg[c];
      *(u32x4_t*)((char*)ldsV(buf) + byte) = vreg[c];
      ba_st_transposed64<T>(ldsKT(buf), row, col8 * 8, kreg[c]);
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
    const int kv0 = t * TILE;
    const bool has_next = (t + 1) < nt;
    u32x4_t kreg[PT], vreg[PT];
    if (has_next) issue_loads(t + 1, kreg, vreg);

    if (!causal || kv0 <= qb + 31) {
      f32x16_t st = (f32x16_t)(0.f), dpt = (f32x16_t)(0.f);
#pragma unroll
      for (int s = 0; s < D / 16; ++s) {
        frag kf = ba_ld_rowslice<T, D, SWZ>(ldsK(cur), l31, 16 * s + 8 * hi);
        frag vf = ba_ld_rowslice<T, D, SWZ>(ldsV(cur), l31, 16 * s + 8 * hi);
        st = MT::mma(kf, qf[s], st);
        dpt = MT::mma(vf, gf[s], dpt);
      }
      // p^T = exp2(S^T c2 - lse2);  dS^T = p^T (dP^T - delta) scale
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kv_g = kv0 + ba_crow(r, 0) + 4 * hi;
        const bool valid =
            kv_g < Sk && (!causal || kv_g <= q_row) && q_row < Sq;
        if constexpr (HAS_CAP) {
          const float t = ba_cap_tanh(st[r], cp.a);
          const float e = valid ? __builtin_fmaf(t, cp.c2, -lse2) : BA_NEG_BIG;
          st[r] = ba_exp2(e) * (dpt[r] - dlt) * __builtin_fmaf(-t, t, 1.f) *
                  scale;
        } else {
          const float e =
              valid ? __builtin_fmaf(st[r], c2, -lse2) : BA_NEG_BIG;
          st[r] = ba_exp2(e) * (dpt[r] - dlt) * scale;
        }
      }
      frag dsf[2];
      ba_build_frag_pair<T>(st, dsf);
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int u = 0; u < 2; ++u)
          dqt[dt] = MT::mma(
              ba_ld_rowslice64<T>(ldsKT(cur), dt * 32 + l31, 16 * u + 8 * hi),
              dsf[u], dqt[dt]);
    }
    if (has_next) write_lds(cur ^ 1, kreg, vreg);
    __syncthreads();
    cur ^= 1;
  }

  if (q_row < Sq) {
    // each (b, q_row, n) row has exactly one writer: a plain read-add-write
    float* drow = dq + b * dq_sb + (int64_t)q_row * dq_ss + n * dq_sh;
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        drow[dt * 32 + ba_crow(r, hi)] += dqt[dt][r];
  }
}

// ============== dV and dK kernels (kv-resident, q/dO streamed) ===========
// MODE 0 (dV): S = mfma(Q, K^T); dV^T += mfma(dO^T, P)
// MODE 1 (dK): + dP = mfma(dO, V^T); dK^T += mfma(Q^T, dS)
// wave w owns kv rows [blk*128 + w*32, +32) of KV head blockIdx.y: the K
// fragments (and V's for dK) and the accumulator stay in registers; the q
// side streams in 32-row tiles, double buffered, as ONE flattened
// (g, tile) stream over the G query heads of the group (G = 1: plain
// multi-head), in a fixed order (g ascending, tiles ascending).  Here the q
// row is the MFMA row axis, so lse * log2e and delta are per-register, not
// per-lane: each tile's 32 + 32 values are staged behind its images and
// read back as 4-float row groups.
template <typename T, int MODE, typename... CAP>
__global__ __launch_bounds__(NT) void bwd_d256_dkv_kernel(
    const T* __restrict__ dout, const T* __restrict__ q,
    const T* __restrict__ k, const T* __restrict__ v,
    const float* __restrict__ delta, const float* __restrict__ lse,
    float* __restrict__ out, int Sq, int Sk, int N, int G,
    int64_t g_sb, int64_t g_ss, int64_t g_sh,
    int64_t q_sb, int64_t q_ss, int64_t q_sh,
    int64_t k_sb, int64_t k_ss, int64_t k_sh,
    int64_t v_sb, int64_t v_ss, int64_t v_sh,
    int64_t d_sb, int64_t d_sh, int64_t l_sb, int64_t l_sh,
    int64_t o_sb, int64_t o_ss, int64_t o_sh,
    float scale, int causal, CAP... cap) {
  using MT = mfma_traits<T>;
  using frag = typename MT::frag;
  constexpr bool HAS_CAP = ba_pack_is<ba_cap_args, CAP...>;
  static_assert(HAS_CAP || sizeof...(CAP) == 0, "the pack: one ba_cap_args");
  ba_cap_args cp = {0.f, 0.f};
  if constexpr (HAS_CAP) cp = ba_cap_of(cap...);
  // images per buffer: dV: [Q row-major | dO^T]; dK: [Q | dO | Q^T]
  constexpr int IMGS = MODE == 0 ? 2 : 3;
  constexpr int ROWC = 2 * TILE * (int)(sizeof(float) / sizeof(T));

  // one LDS object: [2 buffers][IMGS images] [2 buffers][lse2 | delta]
  __shared__ __attribute__((aligned(16))) T lds[2 * IMGS * TILE * D + 2 * ROWC];
  auto ldsQ = [&](int buf) -> T* { return lds + buf * (IMGS * TILE * D); };
  auto ldsG = [&](int buf) -> T* {  // dV: transposed dO; dK: row-major dO
    return lds + buf * (IMGS * TILE * D) + TILE * D;
  };
  auto ldsQT = [&](int buf) -> T* {
    return lds + buf * (IMGS * TILE * D) + 2 * TILE * D;
  };
  auto ldsRow = [&](int buf) -> float* {
    return (float*)(lds + 2 * IMGS * TILE * D) + buf * (2 * TILE);
  };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int n = blockIdx.y, b = blockIdx.z;  // n: the KV head
  const int kvb = blockIdx.x * BA_D256_BLOCK + wave * 32;
  const int kv_col = kvb + l31;

  // the group's first q head; one head stride per g
  const T* qp = q + b * q_sb + (int64_t)n * G * q_sh;
  const T* gp = dout + b * g_sb + (int64_t)n * G * g_sh;
  const float* dp_ = delta + b * d_sb + (int64_t)n * G * d_sh;
  const float* lp_ = lse + b * l_sb + (int64_t)n * G * l_sh;

  frag kf[D / 16], vf[MODE == 1 ? D / 16 : 1];
  {
    const T* kp = k + b * k_sb + (int64_t)n * k_sh;
    const T* vp = v + b * v_sb + (int64_t)n * v_sh;
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      u32x4_t wk = {0, 0, 0, 0}, wv = {0, 0, 0, 0};
      if (kv_col < Sk) {
        wk = *(const u32x4_t*)(kp + (int64_t)kv_col * k_ss + 16 * s + 8 * hi);
        if (MODE == 1)
          wv = *(const u32x4_t*)(vp + (int64_t)kv_col * v_ss + 16 * s + 8 * hi);
      }
      kf[s] = __builtin_bit_cast(frag, wk);
      if (MODE == 1) vf[s] = __builtin_bit_cast(frag, wv);
    }
  }
  const float c2 = scale * BA_LOG2E;

  f32x16_t acc[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) acc[dt] = (f32x16_t)(0.f);

  // causal: q tiles wholly before this workgroup's kv rows are masked
  const int t0 = causal ? (blockIdx.x * BA_D256_BLOCK) / TILE : 0;
  const int nt = (Sq + TILE - 1) / TILE;

  // threads 0..31 carry the tile's lse * log2e rows, 32..63 its delta rows
  auto issue_loads = [&](int g, int tile, u32x4_t* qreg, u32x4_t* greg,
                         float* rowc) {
    const int q0 = tile * TILE;
    const T* qpg = qp + (int64_t)g * q_sh;
    const T* gpg = gp + (int64_t)g * g_sh;
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      const auto [row, col8] = stage_rc(c);
      // clamped, not guarded: rows past Sq re-load row Sq - 1; the
      // q_g < Sq mask zeroes their P / dS
      const int qg = q0 + row;
      const int qc = qg < Sq ? qg : (Sq - 1);
      qreg[c] = *(const u32x4_t*)(qpg + (int64_t)qc * q_ss + col8 * 8);
      greg[c] = *(const u32x4_t*)(gpg + (int64_t)qc * g_ss + col8 * 8);
    }
    if (tid < 2 * TILE) {
      const int qg = q0 + (tid & 31);
      const int qc = qg < Sq ? qg : (Sq - 1);
      if (tid < TILE)
        *rowc = lp_[(int64_t)g * l_sh + qc] * BA_LOG2E;
      else
        *rowc = MODE == 1 ? dp_[(int64_t)g * d_sh + qc] : 0.f;
    }
  };
  auto write_lds = [&](int buf, const u32x4_t* qreg, const u32x4_t* greg,
                       float rowc) {
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      const auto [row, col8] = stage_rc(c);
      const int byte = rowmajor_byte(row, col8);
      *(u32x4_t*)((char*)ldsQ(buf) + byte) = qreg[c];
      if (MODE == 0) {
        ba_st_transposed64<T>(ldsG(buf), row, col8 * 8, greg[c]);
      } else {
        *(u32x4_t*)((char*)ldsG(buf) + byte) = greg[c];
        ba_st_transposed64<T>(ldsQT(buf), row, col8 * 8, qreg[c]);
      }
    }
    if (tid < 2 * TILE) ldsRow(buf)[tid] = rowc;
  };

  {
    u32x4_t qreg[PT], greg[PT];
    float rowc = 0.f;
    issue_loads(0, t0, qreg, greg, &rowc);
    write_lds(0, qreg, greg, rowc);
    __syncthreads();
  }

  int cur = 0;
  for (int g = 0; g < G; ++g)
    for (int t = t0; t < nt; ++t) {
      const int q0 = t * TILE;
      const bool last_t = (t + 1) >= nt;
      const bool has_next = !last_t || g + 1 < G;
      u32x4_t qreg[PT], greg[PT];
      float rowc = 0.f;
      if (has_next)
        issue_loads(last_t ? g + 1 : g, last_t ? t0 : t + 1, qreg, greg, &rowc);

      // causal: this wave's kv rows all lie after the tile's last q row
      if (!causal || q0 + TILE - 1 >= kvb) {
        f32x16_t st = (f32x16_t)(0.f), dpt = (f32x16_t)(0.f);
#pragma unroll
        for (int s = 0; s < D / 16; ++s) {
          st = MT::mma(
              ba_ld_rowslice<T, D, SWZ>(ldsQ(cur), l31, 16 * s + 8 * hi), kf[s],
              st);
          if (MODE == 1)
            dpt = MT::mma(
                ba_ld_rowslice<T, D, SWZ>(ldsG(cur), l31, 16 * s + 8 * hi),
                vf[s], dpt);
        }
        const float* rows = ldsRow(cur);
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          // registers 4 r4 .. 4 r4 + 3 hold q rows 8 r4 + 4 hi + (0..3)
          const float4 l4 = *(const float4*)(rows + 8 * r4 + 4 * hi);
          float4 d4 = make_float4(0.f, 0.f, 0.f, 0.f);
          if (MODE == 1) d4 = *(const float4*)(rows + TILE + 8 * r4 + 4 * hi);
          const float lv[4] = {l4.x, l4.y, l4.z, l4.w};
          const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = 4 * r4 + j;
            const int q_g = q0 + ba_crow(r, 0) + 4 * hi;
            const bool valid =
                q_g < Sq && kv_col < Sk && (!causal || q_g >= kv_col);
            if constexpr (HAS_CAP) {
              const float t = ba_cap_tanh(st[r], cp.a);
              const float e =
                  valid ? __builtin_fmaf(t, cp.c2, -lv[j]) : BA_NEG_BIG;
              const float p = ba_exp2(e);
              st[r] = (MODE == 0) ? p
                                  : p * (dpt[r] - dv[j]) *
                                        __builtin_fmaf(-t, t, 1.f) * scale;
            } else {
              const float e =
                  valid ? __builtin_fmaf(st[r], c2, -lv[j]) : BA_NEG_BIG;
              const float p = ba_exp2(e);
              st[r] = (MODE == 0) ? p : p * (dpt[r] - dv[j]) * scale;  // P : dS
            }
          }
        }
        frag f01[2];
        ba_build_frag_pair<T>(st, f01);
        // A = dO^T (dV) or Q^T (dK) row slice: d row 32 dt + l31
        const T* timg = (MODE == 0) ? ldsG(cur) : ldsQT(cur);
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
          for (int u = 0; u < 2; ++u)
            acc[dt] = MT::mma(
                ba_ld_rowslice64<T>(timg, dt * 32 + l31, 16 * u + 8 * hi),
                f01[u], acc[dt]);
      }
      if (has_next) write_lds(cur ^ 1, qreg, greg, rowc);
      __syncthreads();
      cur ^= 1;
    }

  if (kv_col < Sk) {
    // single writer per (b, kv row, kv head): read-add-write, once per call
    float* row = out + b * o_sb + (int64_t)kv_col * o_ss + n * o_sh;
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        row[dt * 32 + ba_crow(r, hi)] += acc[dt][r];
  }
}

// `cap`: nothing, or the ba_cap_args of a soft-capped kernel
template <typename T, typename K, typename... CAP>
void launch_d256_acc(K kernel, dim3 grid, const bwd_dq_args& a,
                     hipStream_t stream, CAP... cap) {
  kernel<<<grid, dim3(NT), 0, stream>>>(
      (const T*)a.dout, (const T*)a.q, (const T*)a.k, (const T*)a.v, a.delta,
      a.lse, a.out, a.Sq, a.Sk, a.N, a.G, a.g_sb, a.g_ss, a.g_sh, a.q_sb,
      a.q_ss, a.q_sh, a.k_sb, a.k_ss, a.k_sh, a.v_sb, a.v_ss, a.v_sh, a.d_sb,
      a.d_sh, a.l_sb, a.l_sh, a.o_sb, a.o_ss, a.o_sh, a.scale, a.causal,
      cap...);
}

}  // namespace

int ba_d256_bwd(const bwd_dq_args& dq, const bwd_dq_args& dv,
                const bwd_dq_args& dk, int64_t B, int dtype,
                hipStream_t stream) {
  const unsigned qblocks = (unsigned)((dq.Sq + BA_D256_BLOCK - 1) / BA_D256_BLOCK);
  const unsigned kblocks = (unsigned)((dq.Sk + BA_D256_BLOCK - 1) / BA_D256_BLOCK);
  const dim3 qgrid(qblocks, (unsigned)dq.N, (unsigned)B);
  const dim3 kgrid(kblocks, (unsigned)(dq.N / dq.G), (unsigned)B);
  return ba_dispatch_t256(dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    launch_d256_acc<T>(bwd_d256_dq_kernel<T>, qgrid, dq, stream);
    BA_CHECK_LAUNCH();
    launch_d256_acc<T>(bwd_d256_dkv_kernel<T, 0>, kgrid, dv, stream);
    BA_CHECK_LAUNCH();
    launch_d256_acc<T>(bwd_d256_dkv_kernel<T, 1>, kgrid, dk, stream);
    return ba_launch_status();
  });
}

int ba_d256_bwd_cap(const bwd_dq_args& dq, const bwd_dq_args& dv,
                    const bwd_dq_args& dk, const ba_cap_args& cp, int64_t B,
                    int dtype, hipStream_t stream) {
  const unsigned qblocks = (unsigned)((dq.Sq + BA_D256_BLOCK - 1) / BA_D256_BLOCK);
  const unsigned kblocks = (unsigned)((dq.Sk + BA_D256_BLOCK - 1) / BA_D256_BLOCK);
  const dim3 qgrid(qblocks, (unsigned)dq.N, (unsigned)B);
  const dim3 kgrid(kblocks, (unsigned)(dq.N / dq.G), (unsigned)B);
  return ba_dispatch_t256(dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    launch_d256_acc<T>(bwd_d256_dq_kernel<T, ba_cap_args>, qgrid, dq, stream,
                       cp);
    BA_CHECK_LAUNCH();
    launch_d256_acc<T>(bwd_d256_dkv_kernel<T, 0, ba_cap_args>, kgrid, dv,
                       stream, cp);
    BA_CHECK_LAUNCH();
    launch_d256_acc<T>(bwd_d256_dkv_kernel<T, 1, ba_cap_args>, kgrid, dk,
                       stream, cp);
    return ba_launch_status();
  });
}
