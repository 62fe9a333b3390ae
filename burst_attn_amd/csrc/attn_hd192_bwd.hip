// qk head_dim 192 / v head_dim 128 backward tile kernels for gfx950 (design:
// attn_hd192.h), and the backward entry point that takes both widths.
//
// The default "split8" plan of attn_bwd.hip at one wave per SIMD: a
// q-resident dq kernel and the kv-resident dV and dK kernels, each adding
// its tile contribution into a strided fp32 accumulator with one
// read-add-write per owned row and no atomics, so the backward is bitwise
// run-to-run deterministic.  Tile math as at the top of attn_bwd.hip, with
// the width each product is contracted over or written at:
//     s = q k^T (192);  p = exp2(s * c2 - lse * log2e);  dv += p^T do (128)
//     dp = do v^T (128);  ds = p * (dp - delta) * scale
//     dq += ds k (192);   dk += ds^T q (192)
// Streamed tiles are 32 rows (one MFMA subtile).  192-wide row-major images
// have padded 400-byte rows (attn_hd192.h), 128-wide ones the D = 128
// swizzle; the transposed images have 64-byte rows (ba_swz64, attn_d256.h).

#include "attn_hd192.h"
#include "gqa_heads.h"
#include "seg_support.h"

namespace {

constexpr int DQK = BA_HD192_DQK;
constexpr int DV = BA_HD192_DV;
constexpr int NT = BA_HD192_NT;
constexpr int TILE = 32;                      // streamed rows per tile
constexpr int PTQK = (TILE * DQK / 8) / NT;   // 3 chunks per thread
constexpr int PTV = (TILE * DV / 8) / NT;     // 2 chunks per thread
constexpr int IMG_QK = TILE * BA_HD192_ROWB;  // [32][192], padded rows
constexpr int IMG_V = TILE * DV * 2;          // [32][128]
constexpr int IMG_QKT = DQK * TILE * 2;       // [192][32]
constexpr int IMG_VT = DV * TILE * 2;         // [128][32]

// a 16-byte chunk of a 128-wide row-major image (256-byte rows)
__device__ __forceinline__ int rowmajor_v_byte(int row, int col8) {
  return ba_swz<BA_HD192_SWZV>(row * (2 * DV) + col8 * 16, row);
}

// ====================== dq kernel (q-resident) ==========================
// wave w owns q rows [blk*128 + w*32, +32): Q and dO fragments (48 + 32
// dwords) and the dQ^T accumulator (96) stay in registers; K, V and K^T
// tiles of 32 kv rows stream through LDS, double buffered (65 KiB).
//   S^T = mfma(K, Q), 12 k-slices; dP^T = mfma(V, dO), 8 k-slices; dS^T
//   in-lane (lse and delta are lane-local); dQ^T += mfma(K^T, dS^T), 192 rows
template <typename T>
__global__ __launch_bounds__(NT) void bwd_hd192_dq_kernel(
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
    float scale, int causal) {
  using MT = mfma_traits<T>;
  using frag = typename MT::frag;
  constexpr int BUF = IMG_QK + IMG_V + IMG_QKT;

  // [2 buffers][K row-major | V row-major | K^T transposed]
  __shared__ __attribute__((aligned(16))) char lds[2 * BUF];
  auto ldsK = [&](int buf) -> char* { return lds + buf * BUF; };
  auto ldsV = [&](int buf) -> char* { return lds + buf * BUF + IMG_QK; };
  auto ldsKT = [&](int buf) -> T* {
    return (T*)(lds + buf * BUF + IMG_QK + IMG_V);
  };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int n = blockIdx.y, b = blockIdx.z;
  const int qb = blockIdx.x * BA_HD192_BLOCK + wave * 32;
  const int q_row = qb + l31;

  const T* qp = q + b * q_sb + (int64_t)n * q_sh;
  const T* gp = dout + b * g_sb + (int64_t)n * g_sh;
  const int nkv = n / G;  // grouped-query heads: q head n reads n / G
  const T* kp = k + b * k_sb + (int64_t)nkv * k_sh;
  const T* vp = v + b * v_sb + (int64_t)nkv * v_sh;

  frag qf[DQK / 16], gf[DV / 16];
#pragma unroll
  for (int s = 0; s < DQK / 16; ++s) {
    u32x4_t wq = {0, 0, 0, 0};
    if (q_row < Sq)
      wq = *(const u32x4_t*)(qp + (int64_t)q_row * q_ss + 16 * s + 8 * hi);
    qf[s] = __builtin_bit_cast(frag, wq);
  }
#pragma unroll
  for (int s = 0; s < DV / 16; ++s) {
    u32x4_t wg = {0, 0, 0, 0};
    if (q_row < Sq)
      wg = *(const u32x4_t*)(gp + (int64_t)q_row * g_ss + 16 * s + 8 * hi);
    gf[s] = __builtin_bit_cast(frag, wg);
  }
  const float c2 = scale * BA_LOG2E;
  const float lse2 =
      (q_row < Sq) ? lse[b * l_sb + n * l_sh + q_row] * BA_LOG2E : 0.f;
  const float dlt = (q_row < Sq) ? delta[b * d_sb + n * d_sh + q_row] : 0.f;

  f32x16_t dqt[DQK / 32];
#pragma unroll
  for (int dt = 0; dt < DQK / 32; ++dt) dqt[dt] = (f32x16_t)(0.f);

  const int kv_limit =
      causal ? min(Sk, (int)(blockIdx.x + 1) * BA_HD192_BLOCK) : Sk;
  const int nt = (kv_limit + TILE - 1) / TILE;

  // clamped, not guarded: rows past Sk re-load row Sk - 1; their scores are
  // masked to p = 0
  auto issue_loads = [&](int tile, u32x4_t* kreg, u32x4_t* vreg) {
#pragma unroll
    for (int c = 0; c < PTQK; ++c) {
      const auto [row, col8] = ba_hd192_rc_qk(c);
      const int kvg = tile * TILE + row;
      const int kvc = kvg < Sk ? kvg : (Sk - 1);
      kreg[c] = *(const u32x4_t*)(kp + (int64_t)kvc * k_ss + col8 * 8);
    }
#pragma unroll
    for (int c = 0; c < PTV; ++c) {
      const auto [row, col8] = ba_hd192_rc_v(c);
      const int kvg = tile * TILE + row;
      const int kvc = kvg < Sk ? kvg : (Sk - 1);
      vreg[c] = *(const u32x4_t*)(vp + (int64_t)kvc * v_ss + col8 * 8);
    }
  };
  auto write_lds = [&](int buf, const u32x4_t* kreg, const u32x4_t* vreg) {
#pragma unroll
    for (int c = 0; c < PTQK; ++c) {
      const auto [row, col8] = ba_hd192_rc_qk(c);
      ba_st_row192(ldsK(buf), row, col8, kreg[c]);
      ba_st_transposed64<T>(ldsKT(buf), row, col8 * 8, kreg[c]);
    }
#pragma unroll
    for (int c = 0; c < PTV; ++c) {
      const auto [row, col8] = ba_hd192_rc_v(c);
      *(u32x4_t*)(ldsV(buf) + rowmajor_v_byte(row, col8)) = vreg[c];
    }
  };

  {
    u32x4_t kreg[PTQK], vreg[PTV];
    issue_loads(0, kreg, vreg);
    write_lds(0, kreg, vreg);
    __syncthreads();
  }

  int cur = 0;
  for (int t = 0; t < nt; ++t) {
    const int kv0 = t * TILE;
    const bool has_next = (t + 1) < nt;
    u32x4_t kreg[PTQK], vreg[PTV];
    if (has_next) issue_loads(t + 1, kreg, vreg);

    if (!causal || kv0 <= qb + 31) {
      f32x16_t st = (f32x16_t)(0.f), dpt = (f32x16_t)(0.f);
#pragma unroll
      for (int s = 0; s < DQK / 16; ++s)
        st = MT::mma(ba_ld_row192<T>(ldsK(cur), l31, 16 * s + 8 * hi), qf[s],
                     st);
#pragma unroll
      for (int s = 0; s < DV / 16; ++s)
        dpt = MT::mma(ba_ld_rowslice<T, DV, BA_HD192_SWZV>(
                          (const T*)ldsV(cur), l31, 16 * s + 8 * hi),
                      gf[s], dpt);
      // p^T = exp2(S^T c2 - lse2);  dS^T = p^T (dP^T - delta) scale
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kv_g = kv0 + ba_crow(r, 0) + 4 * hi;
        const bool valid =
            kv_g < Sk && (!causal || kv_g <= q_row) && q_row < Sq;
        const float e = valid ? __builtin_fmaf(st[r], c2, -lse2) : BA_NEG_BIG;
        st[r] = ba_exp2(e) * (dpt[r] - dlt) * scale;
      }
      frag dsf[2];
      ba_build_frag_pair<T>(st, dsf);
#pragma unroll
      for (int dt = 0; dt < DQK / 32; ++dt)
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
    for (int dt = 0; dt < DQK / 32; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        drow[dt * 32 + ba_crow(r, hi)] += dqt[dt][r];
  }
}

// ============== dV and dK kernels (kv-resident, q/dO streamed) ===========
// MODE 0 (dV): S = mfma(Q, K^T) over 192; dV^T += mfma(dO^T, P), 128 rows
// MODE 1 (dK): + dP = mfma(dO, V^T) over 128; dK^T += mfma(Q^T, dS), 192 rows
// wave w owns kv rows [blk*128 + w*32, +32) of KV head blockIdx.y: the K
// fragments (and V's for dK) and the accumulator stay in registers; the q
// side streams in 32-row tiles, double buffered, as ONE flattened
// (g, tile) stream over the G query heads of the group (G = 1: plain
// multi-head), in a fixed order (g ascending, tiles ascending).  The q row
// is the MFMA row axis here, so lse * log2e and delta are per-register: each
// tile's 32 + 32 values are staged behind its images and read back as
// 4-float row groups.
template <typename T, int MODE>
__global__ __launch_bounds__(NT) void bwd_hd192_dkv_kernel(
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
    float scale, int causal) {
  using MT = mfma_traits<T>;
  using frag = typename MT::frag;
  // images per buffer: dV: [Q row-major | dO^T]; dK: [Q | dO | Q^T]
  constexpr int BUF = MODE == 0 ? IMG_QK + IMG_VT : IMG_QK + IMG_V + IMG_QKT;
  constexpr int DOUT = MODE == 0 ? DV : DQK;  // width of the accumulator

  // one LDS object: [2 buffers][images] [2 buffers][lse2 | delta]
  __shared__ __attribute__((aligned(16))) char
      lds[2 * BUF + 2 * 2 * TILE * (int)sizeof(float)];
  auto ldsQ = [&](int buf) -> char* { return lds + buf * BUF; };
  auto ldsG = [&](int buf) -> char* {  // dV: transposed dO; dK: row-major dO
    return lds + buf * BUF + IMG_QK;
  };
  auto ldsQT = [&](int buf) -> T* {
    return (T*)(lds + buf * BUF + IMG_QK + IMG_V);
  };
  auto ldsRow = [&](int buf) -> float* {
    return (float*)(lds + 2 * BUF) + buf * (2 * TILE);
  };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int n = blockIdx.y, b = blockIdx.z;  // n: the KV head
  const int kvb = blockIdx.x * BA_HD192_BLOCK + wave * 32;
  const int kv_col = kvb + l31;

  // the group's first q head; one head stride per g
  const T* qp = q + b * q_sb + (int64_t)n * G * q_sh;
  const T* gp = dout + b * g_sb + (int64_t)n * G * g_sh;
  const float* dp_ = delta + b * d_sb + (int64_t)n * G * d_sh;
  const float* lp_ = lse + b * l_sb + (int64_t)n * G * l_sh;

  frag kf[DQK / 16], vf[MODE == 1 ? DV / 16 : 1];
  {
    const T* kp = k + b * k_sb + (int64_t)n * k_sh;
    const T* vp = v + b * v_sb + (int64_t)n * v_sh;
#pragma unroll
    for (int s = 0; s < DQK / 16; ++s) {
      u32x4_t wk = {0, 0, 0, 0};
      if (kv_col < Sk)
        wk = *(const u32x4_t*)(kp + (int64_t)kv_col * k_ss + 16 * s + 8 * hi);
      kf[s] = __builtin_bit_cast(frag, wk);
    }
    if (MODE == 1) {
#pragma unroll
      for (int s = 0; s < DV / 16; ++s) {
        u32x4_t wv = {0, 0, 0, 0};
        if (kv_col < Sk)
          wv = *(const u32x4_t*)(vp + (int64_t)kv_col * v_ss + 16 * s + 8 * hi);
        vf[s] = __builtin_bit_cast(frag, wv);
      }
    }
  }
  const float c2 = scale * BA_LOG2E;

  f32x16_t acc[DOUT / 32];
#pragma unroll
  for (int dt = 0; dt < DOUT / 32; ++dt) acc[dt] = (f32x16_t)(0.f);

  // causal: q tiles wholly before this workgroup's kv rows are masked
  const int t0 = causal ? (blockIdx.x * BA_HD192_BLOCK) / TILE : 0;
  const int nt = (Sq + TILE - 1) / TILE;

  // threads 0..31 carry the tile's lse * log2e rows, 32..63 its delta rows;
  // clamped, not guarded: rows past Sq re-load row Sq - 1 and the q_g < Sq
  // mask zeroes their P / dS
  auto issue_loads = [&](int g, int tile, u32x4_t* qreg, u32x4_t* greg,
                         float* rowc) {
    const int q0 = tile * TILE;
    const T* qpg = qp + (int64_t)g * q_sh;
    const T* gpg = gp + (int64_t)g * g_sh;
#pragma unroll
    for (int c = 0; c < PTQK; ++c) {
      const auto [row, col8] = ba_hd192_rc_qk(c);
      const int qg = q0 + row;
      const int qc = qg < Sq ? qg : (Sq - 1);
      qreg[c] = *(const u32x4_t*)(qpg + (int64_t)qc * q_ss + col8 * 8);
    }
#pragma unroll
    for (int c = 0; c < PTV; ++c) {
      const auto [row, col8] = ba_hd192_rc_v(c);
      const int qg = q0 + row;
      const int qc = qg < Sq ? qg : (Sq - 1);
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
    for (int c = 0; c < PTQK; ++c) {
      const auto [row, col8] = ba_hd192_rc_qk(c);
      ba_st_row192(ldsQ(buf), row, col8, qreg[c]);
      if (MODE == 1) ba_st_transposed64<T>(ldsQT(buf), row, col8 * 8, qreg[c]);
    }
#pragma unroll
    for (int c = 0; c < PTV; ++c) {
      const auto [row, col8] = ba_hd192_rc_v(c);
      if (MODE == 0)
        ba_st_transposed64<T>((T*)ldsG(buf), row, col8 * 8, greg[c]);
      else
        *(u32x4_t*)(ldsG(buf) + rowmajor_v_byte(row, col8)) = greg[c];
    }
    if (tid < 2 * TILE) ldsRow(buf)[tid] = rowc;
  };

  {
    u32x4_t qreg[PTQK], greg[PTV];
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
      u32x4_t qreg[PTQK], greg[PTV];
      float rowc = 0.f;
      if (has_next)
        issue_loads(last_t ? g + 1 : g, last_t ? t0 : t + 1, qreg, greg, &rowc);

      // causal: this wave's kv rows all lie after the tile's last q row
      if (!causal || q0 + TILE - 1 >= kvb) {
        f32x16_t st = (f32x16_t)(0.f), dpt = (f32x16_t)(0.f);
#pragma unroll
        for (int s = 0; s < DQK / 16; ++s)
          st = MT::mma(ba_ld_row192<T>(ldsQ(cur), l31, 16 * s + 8 * hi), kf[s],
                       st);
        if (MODE == 1) {
#pragma unroll
          for (int s = 0; s < DV / 16; ++s)
            dpt = MT::mma(ba_ld_rowslice<T, DV, BA_HD192_SWZV>(
                              (const T*)ldsG(cur), l31, 16 * s + 8 * hi),
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
            const float e =
                valid ? __builtin_fmaf(st[r], c2, -lv[j]) : BA_NEG_BIG;
            const float p = ba_exp2(e);
            st[r] = (MODE == 0) ? p : p * (dpt[r] - dv[j]) * scale;  // P : dS
          }
        }
        frag f01[2];
        ba_build_frag_pair<T>(st, f01);
        // A = dO^T (dV) or Q^T (dK) row slice: channel 32 dt + l31
        const T* timg = (MODE == 0) ? (const T*)ldsG(cur) : ldsQT(cur);
#pragma unroll
        for (int dt = 0; dt < DOUT / 32; ++dt)
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
    for (int dt = 0; dt < DOUT / 32; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        row[dt * 32 + ba_crow(r, hi)] += acc[dt][r];
  }
}

template <typename T, typename K>
void launch_hd192_acc(K kernel, dim3 grid, const bwd_dq_args& a,
                      hipStream_t stream) {
  kernel<<<grid, dim3(NT), 0, stream>>>(
      (const T*)a.dout, (const T*)a.q, (const T*)a.k, (const T*)a.v, a.delta,
      a.lse, a.out, a.Sq, a.Sk, a.N, a.G, a.g_sb, a.g_ss, a.g_sh, a.q_sb,
      a.q_ss, a.q_sh, a.k_sb, a.k_ss, a.k_sh, a.v_sb, a.v_ss, a.v_sh, a.d_sb,
      a.d_sh, a.l_sb, a.l_sh, a.o_sb, a.o_ss, a.o_sh, a.scale, a.causal);
}

}  // namespace

extern "C" int bahip_attn_bwd_dv(
    const void* dout, const void* q, const void* k, const void* v,
    const float* delta, const float* lse, float* dq, float* dk, float* dv,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    int64_t Dv, const int64_t gs[3], const int64_t qs[3], const int64_t ks[3],
    const int64_t vs[3], const int64_t ds[2], const int64_t ls[2],
    const int64_t dqs[3], const int64_t dks[3], const int64_t dvs[3],
    float scale, int causal, int deterministic, int dtype, void* stream) {
  int same;
  if (int rc = ba_hd192_route(D, Dv, &same)) return rc;
  if (same)
    return bahip_attn_bwd_gqa(dout, q, k, v, delta, lse, dq, dk, dv, B, Sq, Sk,
                              N, Nk, D, gs, qs, ks, vs, ds, ls, dqs, dks, dvs,
                              scale, causal, deterministic, dtype, stream);
  // The (192, 128) backward: the default plan's three kernels only; every
  // refusal comes before the first launch.
  (void)deterministic;  // deterministic by construction
  if (causal && Sq != Sk)
    return ba_fail(BAHIP_ERR_CAUSAL_SHAPE,
                   "causal tiles require Sq == Sk (%d vs %d)", (int)Sq,
                   (int)Sk);
  const int G = (int)ba_gqa_group(N, Nk);
  if (!G)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "q heads N=%d must be a positive multiple of kv heads "
                   "Nk=%d",
                   (int)N, (int)Nk);
  ba_bwd_knobs kn;
  kn.fused = ba_env_int(BA_BWD_KNOB_SPECS[0].env, kn.fused);
  kn.dk_flip = ba_env_int(BA_BWD_KNOB_SPECS[1].env, kn.dk_flip);
  kn.dq_pipe = ba_env_int(BA_BWD_KNOB_SPECS[2].env, kn.dq_pipe);
  kn.dkq_dbg = ba_env_int(BA_BWD_KNOB_SPECS[3].env, kn.dkq_dbg);
  const ba_bwd_plan plan = ba_bwd_select(kn, G);
  if (plan.verdict == BA_BWD_BAD_VALUE)
    return ba_fail(BAHIP_ERR_BAD_KNOB, "%s=%d is not an accepted value",
                   plan.knob, plan.value);
  const ba_seg_verdict sv = ba_seg_bwd_support(kn);
  if (sv.knob)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "%s=%d does not support head_dim pair (192, 128) (default "
                   "backward plan only)",
                   sv.knob, sv.value);
  if (B < 1 || B > 65535 || N > 65535 || Sq < 1 || Sk < 1)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "head_dim pair (192, 128): unsupported shape B=%d Sq=%d "
                   "Sk=%d N=%d",
                   (int)B, (int)Sq, (int)Sk, (int)N);
  const auto acc_into = [&](float* out, const int64_t* os) -> bwd_dq_args {
    return {dout, q, k, v, delta, lse, out, (int)Sq, (int)Sk, (int)N, G,
            gs[0], gs[1], gs[2], qs[0], qs[1], qs[2], ks[0], ks[1], ks[2],
            vs[0], vs[1], vs[2], ds[0], ds[1], ls[0], ls[1],
            os[0], os[1], os[2], scale, causal};
  };
  const bwd_dq_args dqa = acc_into(dq, dqs), dva = acc_into(dv, dvs),
                    dka = acc_into(dk, dks);
  const unsigned qblocks = (unsigned)((Sq + BA_HD192_BLOCK - 1) / BA_HD192_BLOCK);
  const unsigned kblocks = (unsigned)((Sk + BA_HD192_BLOCK - 1) / BA_HD192_BLOCK);
  const dim3 qgrid(qblocks, (unsigned)N, (unsigned)B);
  const dim3 kgrid(kblocks, (unsigned)Nk, (unsigned)B);
  const hipStream_t st = (hipStream_t)stream;
  return ba_dispatch_t192(dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    launch_hd192_acc<T>(bwd_hd192_dq_kernel<T>, qgrid, dqa, st);
    BA_CHECK_LAUNCH();
    launch_hd192_acc<T>(bwd_hd192_dkv_kernel<T, 0>, kgrid, dva, st);
    BA_CHECK_LAUNCH();
    launch_hd192_acc<T>(bwd_hd192_dkv_kernel<T, 1>, kgrid, dka, st);
    return ba_launch_status();
  });
}
