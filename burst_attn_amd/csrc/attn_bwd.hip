// BurstAttention backward tile kernels for gfx950 (MI355X, CDNA4).
//
// Replaces the flash-attn backward the reference calls at
// burst_attn/burst_utils.py:211-248, with the tile math of the reference's
// own restatement (burst_utils.py:77-101):
//     p   = exp(q k^T * scale - lse)
//     dv += p^T do;   dp = do v^T;   ds = p * (dp - delta) * scale
//     dq += ds k;     dk += ds^T q
//
// dq/dk/dv are fp32 ACCUMULATORS: every kernel adds its tile contribution
// in place (strided), which lets the ring layer accumulate across rounds
// with no elementwise-add passes or per-round allocations.
//
// Kernel plans behind bahip_attn_bwd (selection: bwd_plans.h; the
// `deterministic` argument does not choose between them):
//   default "split8" (atomic-free, 8 tile GEMMs — flash-attn executes 5):
//     1. bwd_preprocess: delta = rowsum(o * do) fp32  (flash's preprocess)
//     2. dq kernel  (8 waves, q-block resident, streams k/v):
//          S^T = mfma(K,Q); dP^T = mfma(V,dO); dS^T in-lane;
//          dQ^T += mfma(K^T, dS^T)          — all softmax state lane-local
//     3. dkdv kernels (kv-block resident, streams q/do):
//          MODE 0 (dV): S = mfma(Q,K^T); dV^T += mfma(dO^T, P)
//          MODE 1 (dK): + dP = mfma(dO,V^T); dK^T += mfma(Q^T, dS)
//   BA_BWD_FUSED=1 "dkvf7" (7 GEMMs, atomic-free): dq kernel + the fused
//     flipped dK+dV kernel (bwd_dkq_kernel FUSE_DV=1, described above it)
//   BA_BWD_FUSED=2 "atomic6" (6 GEMMs — the flash-attn plan): the fused
//     dK+dQ kernel (bwd_dkq_kernel FUSE_DQ=1, fp32 atomic dq) + dkdv MODE 0
// Operand scheme and LDS swizzle: see attn_common.h.

#include "attn_common.h"
#include "attn_host.h"
#include "bwd_plans.h"
#include "gqa_heads.h"
#include "seg_support.h"

namespace {

// ====================== delta preprocess ==============================
template <typename T, int D>
__global__ __launch_bounds__(256) void bwd_preprocess_kernel(
    const T* __restrict__ o, const T* __restrict__ dout,
    float* __restrict__ delta, int S, int N,
    int64_t o_sb, int64_t o_ss, int64_t o_sh,
    int64_t g_sb, int64_t g_ss, int64_t g_sh) {
  // one wave: 8 rows x 8 lanes/row, 16B..32B per lane
  constexpr int EPL = D / 8;  // elements per lane (16 for D=128)
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int row_in = wave * 8 + (lane >> 3);
  const int sub = lane & 7;
  const int s = blockIdx.x * 32 + row_in;
  const int n = blockIdx.y, b = blockIdx.z;
  if (s >= S) return;
  const T* op = o + b * o_sb + (int64_t)s * o_ss + n * o_sh + sub * EPL;
  const T* gp = dout + b * g_sb + (int64_t)s * g_ss + n * g_sh + sub * EPL;
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < EPL; ++j) acc += (float)op[j] * (float)gp[j];
  acc += __shfl_xor(acc, 1);
  acc += __shfl_xor(acc, 2);
  acc += __shfl_xor(acc, 4);
  if (sub == 0) delta[((int64_t)b * N + n) * S + s] = acc;
}

// ====================== dq kernel (q-resident) ========================
constexpr int KVBLK = 64;

// DQP=1 (env BA_DQ_PIPE): register-relief + explicit read-ahead
// experiment driven by the r2 wait-taxonomy finding: the
// dO fragments move from 32 registers to a persistent LDS image, and
// the freed registers hold a 2-deep software pipeline of the k/v
// fragment reads so each ds_read has >= 2 MFMAs of cover.
// SEG: empty = the plain kernel; one ba_seg_args = the segment-id form
// (attn_common.h; the forward's rules: id equality in `valid`, the block's
// kv tile range from the pre-pass, per-wave tile skip by (min, max), an
// empty range leaves before the first barrier having added nothing).
template <typename T, int D, int DQP = 0, typename... SEG>
__global__ __launch_bounds__(512) void bwd_dq_kernel(
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
    float scale, int causal, SEG... seg) {
  using MT = mfma_traits<T>;
  using frag = typename MT::frag;
  constexpr bool HAS_BAND = ba_pack_is<ba_band_args, SEG...>;
  constexpr bool HAS_SEG = sizeof...(SEG) != 0 && !HAS_BAND;
  constexpr bool HAS_MASK = HAS_SEG || HAS_BAND;
  static_assert(!HAS_MASK || (sizeof...(SEG) == 1 && DQP == 0),
                "segment ids / band: the default dq kernel");
  // band form: the band is the whole mask (the launcher folded causal in)
  if constexpr (HAS_BAND) causal = 0;
  constexpr int SWZ = (D == 128) ? 15 : 7;   // row-major images (2*D B rows)
  constexpr int SWZ_T = 7;                   // transposed images (128 B rows)
  constexpr int NT = 512;
  constexpr int PT = (KVBLK * D / 8) / NT;

  // [2 buffers][K row-major | V row-major | K^T transposed]
  // (+ DQP: persistent dO image for the workgroup's 256 q rows)
  __shared__ T lds[2 * 3 * KVBLK * D + (DQP ? 256 * D : 0)];
  auto ldsK = [&](int buf) -> T* { return lds + buf * (3 * KVBLK * D); };
  auto ldsV = [&](int buf) -> T* { return lds + buf * (3 * KVBLK * D) + KVBLK * D; };
  auto ldsKT = [&](int buf) -> T* { return lds + buf * (3 * KVBLK * D) + 2 * KVBLK * D; };
  T* ldsDO = lds + 2 * 3 * KVBLK * D;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int n = blockIdx.y, b = blockIdx.z;
  const int qb = blockIdx.x * 256 + wave * 32;
  const int q_row = qb + l31;

  const T* qp = q + b * q_sb + (int64_t)n * q_sh;
  const T* gp = dout + b * g_sb + (int64_t)n * g_sh;
  // grouped-query heads: q head n reads KV head n / G (wave-uniform)
  const int nkv = n / G;
  const T* kp = k + b * k_sb + (int64_t)nkv * k_sh;
  const T* vp = v + b * v_sb + (int64_t)nkv * v_sh;

  frag qf[D / 16], gf[DQP ? 1 : D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    if (q_row < Sq) {
      qf[s] = __builtin_bit_cast(
          frag, *(const u32x4_t*)(qp + (int64_t)q_row * q_ss + 16 * s + 8 * hi));
      if (!DQP)
        gf[s] = __builtin_bit_cast(
            frag,
            *(const u32x4_t*)(gp + (int64_t)q_row * g_ss + 16 * s + 8 * hi));
    } else {
      u32x4_t z = {0, 0, 0, 0};
      qf[s] = __builtin_bit_cast(frag, z);
      if (!DQP) gf[s] = __builtin_bit_cast(frag, z);
    }
  }
  if (DQP) {
    // one-time: stage the workgroup's dO block [256 q][D] row-major
    // (clamped rows contribute garbage x 0 through the q_row mask)
    constexpr int PTD = (256 * D / 8) / NT;
#pragma unroll
    for (int c = 0; c < PTD; ++c) {
      const int flat = tid + c * NT;
      const int row = flat / (D / 8), col8 = flat % (D / 8);
      const int qg = blockIdx.x * 256 + row;
      const int qc = qg < Sq ? qg : (Sq - 1);
      u32x4_t ch = *(const u32x4_t*)(gp + (int64_t)qc * g_ss + col8 * 8);
      const int byte = ba_swz<SWZ>(row * (2 * D) + col8 * 16, row);
      *(u32x4_t*)((char*)ldsDO + byte) = ch;
    }
  }
  const float c2 = scale * BA_LOG2E;
  const float lse2 =
      (q_row < Sq) ? lse[b * l_sb + n * l_sh + q_row] * BA_LOG2E : 0.f;
  const float dlt =
      (q_row < Sq) ? delta[b * d_sb + n * d_sh + q_row] : 0.f;

  f32x16_t dqt[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) dqt[dt] = (f32x16_t)(0.f);

  const int kv_limit = causal ? min(Sk, (int)(blockIdx.x + 1) * 256) : Sk;
  const int nt_shape = (kv_limit + KVBLK - 1) / KVBLK;
  int2 trange = {0, nt_shape};
  int qid = 0, wq_min = 0, wq_max = 0;
  const int32_t* kseg = nullptr;
  const int2* tmm = nullptr;
  if constexpr (HAS_SEG) {
    const ba_seg_args sg = ba_seg_of(seg...);
    const int2 r = sg.blk_range[(int64_t)b * gridDim.x + blockIdx.x];
    trange.x = r.x;
    trange.y = min(trange.y, r.y);
    if (trange.x >= trange.y) return;  // workgroup-uniform, no barrier yet
    qid = sg.q_seg[b * sg.q_sb + min(q_row, Sq - 1)];
    ba_wave_minmax(qid, wq_min, wq_max);
    kseg = sg.kv_seg + b * sg.kv_sb;
    tmm = sg.tile_mm + (int64_t)b * ((Sk + KVBLK - 1) / KVBLK);
  }
  // band form: the block's kv tile range is arithmetic (band_support.h)
  ba_band_args bd = {0, 0};
  if constexpr (HAS_BAND) {
    static_assert(KVBLK == BA_BAND_TILE, "band: tiles of band_support.h");
    bd = ba_band_of(seg...);
    const ba_tile_range r = ba_band_block_tiles(blockIdx.x, bd, Sq, Sk);
    trange.x = r.lo;
    trange.y = r.hi;
    if (trange.x >= trange.y) return;  // workgroup-uniform, no barrier yet
  }
  const int t_first = HAS_MASK ? trange.x : 0;
  const int nt = HAS_MASK ? trange.y : nt_shape;

  auto issue_loads = [&](int tile, u32x4_t* kreg, u32x4_t* vreg) {
    const int kv0 = tile * KVBLK;
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      const int flat = tid + c * NT;
      const int row = flat / (D / 8), col8 = flat % (D / 8);
      // clamped instead of guarded (see attn_fwd.hip): out-of-range kv
      // rows re-load row Sk-1; their S values are masked to p = 0
      const int kvg = kv0 + row;
      const int kvc = kvg < Sk ? kvg : (Sk - 1);
      kreg[c] = *(const u32x4_t*)(kp + (int64_t)kvc * k_ss + col8 * 8);
      vreg[c] = *(const u32x4_t*)(vp + (int64_t)kvc * v_ss + col8 * 8);
    }
  };
  auto write_lds = [&](int buf, const u32x4_t* kreg, const u32x4_t* vreg) {
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      const int flat = tid + c * NT;
      const int row = flat / (D / 8), col8 = flat % (D / 8);
      const int byte = ba_swz<SWZ>(row * (2 * D) + col8 * 16, row);
      *(u32x4_t*)((char*)ldsK(buf) + byte) = kreg[c];
      *(u32x4_t*)((char*)ldsV(buf) + byte) = vreg[c];
      ba_st_transposed<T, KVBLK, SWZ_T, 7>(ldsKT(buf), row, col8 * 8, kreg[c]);
    }
  };

  {
    u32x4_t kreg[PT], vreg[PT];
    issue_loads(t_first, kreg, vreg);
    write_lds(0, kreg, vreg);
    __syncthreads();
  }
  if (__builtin_amdgcn_readfirstlane(threadIdx.x) >= 256)
    __builtin_amdgcn_s_setprio(1);  // T5 static form (younger half)

  int cur = 0;
  for (int t = t_first; t < nt; ++t) {
    const int kv0 = t * KVBLK;
    const bool has_next = (t + 1) < nt;
    u32x4_t kreg[PT], vreg[PT];
    if (has_next) issue_loads(t + 1, kreg, vreg);

    bool active, seg_mask = false;
    if constexpr (HAS_SEG) {
      // segment form: the tile's (min, max) ids against the wave's
      const int2 mm = tmm[t];
      seg_mask = !(mm.x == mm.y && wq_min == wq_max && mm.x == wq_min);
      active = (!causal || (kv0 <= qb + 31)) && mm.y >= wq_min &&
               mm.x <= wq_max;
    } else if constexpr (HAS_BAND) {
      active = ba_band_wave_active(qb, kv0, bd);
    } else {
      active = !causal || (kv0 <= qb + 31);
    }
    if (active) {
#pragma unroll
      for (int kvs = 0; kvs < 2; ++kvs) {
        f32x16_t st = (f32x16_t)(0.f), dpt = (f32x16_t)(0.f);
        if (DQP) {
          // explicit 2-deep read-ahead: fragment reads for slice s+1
          // issue before slice s's MFMAs, so each ds_read is covered by
          // >= 2 MFMAs instead of the allocator's read-wait-use
          frag kfA = ba_ld_rowslice<T, D, SWZ>(ldsK(cur), kvs * 32 + l31,
                                               8 * hi);
          frag vfA = ba_ld_rowslice<T, D, SWZ>(ldsV(cur), kvs * 32 + l31,
                                               8 * hi);
          frag gfA = ba_ld_rowslice<T, D, SWZ>(ldsDO, wave * 32 + l31,
                                               8 * hi);
#pragma unroll
          for (int s = 0; s < D / 16; ++s) {
            frag kfB = kfA, vfB = vfA, gfB = gfA;
            if (s + 1 < D / 16) {
              kfA = ba_ld_rowslice<T, D, SWZ>(ldsK(cur), kvs * 32 + l31,
                                              16 * (s + 1) + 8 * hi);
              vfA = ba_ld_rowslice<T, D, SWZ>(ldsV(cur), kvs * 32 + l31,
                                              16 * (s + 1) + 8 * hi);
              gfA = ba_ld_rowslice<T, D, SWZ>(ldsDO, wave * 32 + l31,
                                              16 * (s + 1) + 8 * hi);
            }
            st = MT::mma(kfB, qf[s], st);
            dpt = MT::mma(vfB, gfB, dpt);
          }
        } else {
#pragma unroll
        for (int s = 0; s < D / 16; ++s) {
          frag kf = ba_ld_rowslice<T, D, SWZ>(ldsK(cur), kvs * 32 + l31,
                                              16 * s + 8 * hi);
          frag vf = ba_ld_rowslice<T, D, SWZ>(ldsV(cur), kvs * 32 + l31,
                                              16 * s + 8 * hi);
          st = MT::mma(kf, qf[s], st);
          dpt = MT::mma(vf, gf[DQP ? 0 : s], dpt);
        }
        }
        // p^T = exp2(S^T*c2 - lse2);  dS^T = p^T*(dP^T - delta)*scale
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv_g = kv0 + kvs * 32 + ba_crow(r, 0) + 4 * hi;
          bool valid =
              kv_g < Sk && (!causal || kv_g <= q_row) && q_row < Sq;
          if constexpr (HAS_SEG)
            valid = valid && (!seg_mask || kseg[min(kv_g, Sk - 1)] == qid);
          if constexpr (HAS_BAND)
            valid = valid && ba_band_visible(q_row, kv_g, bd);
          const float e = valid ? __builtin_fmaf(st[r], c2, -lse2) : BA_NEG_BIG;
          const float p = ba_exp2(e);
          st[r] = p * (dpt[r] - dlt) * scale;
        }
        frag dsf[2];
        ba_build_frag_pair<T>(st, dsf);
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt) {
          const int col = dt * 32 + l31;
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            frag ktf = ba_ld_rowslice<T, KVBLK, SWZ_T, 7>(
                ldsKT(cur), col, kvs * 32 + 16 * u + 8 * hi);
            dqt[dt] = MT::mma(ktf, dsf[u], dqt[dt]);
          }
        }
      }
    }
    if (has_next) write_lds(cur ^ 1, kreg, vreg);
    __syncthreads();
    cur ^= 1;
  }

  if (q_row < Sq) {
    // accumulate epilogue: each (b, q_row, n) row is written by exactly
    // one lane, so a plain read-add-write stays deterministic
    float* drow = dq + b * dq_sb + (int64_t)q_row * dq_ss + n * dq_sh;
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        drow[dt * 32 + ba_crow(r, hi)] += dqt[dt][r];
  }
}

// ============== dk and dv kernels (kv-resident, q/do streamed) =========
// Two single-purpose 8-wave kernels instead of one fused dk+dv kernel:
// the fused form needs 4 x 64 accumulator registers per lane and spilled
// (~90 VGPRs) at the 2-waves/SIMD budget; split, each kernel is register
// -clean and runs at the dq kernel's rate.  Cost: S is recomputed (the
// backward executes 8 tile GEMMs total vs flash-attn's 5).
// MODE: 0 = dV (dv^T += mfma(dO^T, P)); 1 = dK (dk^T += mfma(Q^T, dS)).
// QBLK: streamed q-tile rows (128 for dV measured -8%: 27-VGPR spills).
// GQA: 0 = one q head per workgroup (blockIdx.y = q head = kv head; G is
//   ignored) — the equal-heads kernel, unchanged.
//   1 = grouped-query heads: blockIdx.y is the KV head and the workgroup
//   streams the q/dO/lse/delta tiles of its G query heads
//   (heads blockIdx.y*G .. +G-1) through the same double-buffered
//   pipeline as ONE flattened (g, tile) stream: the prefetch of head
//   g+1's first tile overlaps head g's last tile, K/V fragments and the
//   accumulator stay resident, and the epilogue is still one
//   read-add-write per kv row.  Summation order is fixed (g ascending,
//   tiles ascending), so the result stays bitwise deterministic.  A
//   template parameter rather than a runtime G = 1 so the equal-heads
//   instantiation keeps its register allocation (the dK kernel is tight).
// SEG: empty = the plain kernel; one ba_seg_args = the segment-id form
// (attn_common.h), the dq kernel's with the sides swapped: the lane's kv id
// against the q ids of a tile, the block's q tile range from the pre-pass
// (the same for every member of a group, so the flattened stream and its
// "next head's first tile" prefetch only see another t0 and nt).
template <typename T, int D, int MODE, int QBLK = 64, int GQA = 0,
          typename... SEG>
__global__ __launch_bounds__(512) void bwd_dkv_kernel(
    const T* __restrict__ dout, const T* __restrict__ q,
    const T* __restrict__ k, const T* __restrict__ v,
    const float* __restrict__ delta, const float* __restrict__ lse,
    float* __restrict__ dout_acc, int Sq, int Sk, int N, int G,
    int64_t g_sb, int64_t g_ss, int64_t g_sh,
    int64_t q_sb, int64_t q_ss, int64_t q_sh,
    int64_t k_sb, int64_t k_ss, int64_t k_sh,
    int64_t v_sb, int64_t v_ss, int64_t v_sh,
    int64_t d_sb, int64_t d_sh, int64_t l_sb, int64_t l_sh,
    int64_t o_sb, int64_t o_ss, int64_t o_sh,
    float scale, int causal, SEG... seg) {
  using MT = mfma_traits<T>;
  using frag = typename MT::frag;
  constexpr bool HAS_BAND = ba_pack_is<ba_band_args, SEG...>;
  constexpr bool HAS_SEG = sizeof...(SEG) != 0 && !HAS_BAND;
  constexpr bool HAS_MASK = HAS_SEG || HAS_BAND;
  static_assert(!HAS_MASK || (sizeof...(SEG) == 1 && QBLK == BA_SEG_TILE &&
                              QBLK == BA_BAND_TILE),
                "segment ids / band: q tiles of the pre-pass's tile size");
  // band form: the band is the whole mask (the launcher folded causal in)
  if constexpr (HAS_BAND) causal = 0;
  constexpr int SWZ = (D == 128) ? 15 : 7;
  constexpr int SWZ_T = 7;
  constexpr int NT = 512;
  constexpr int PT = (QBLK * D / 8) / NT;
  // images per buffer: MODE_DV: [Q row-major | dO^T]; MODE_DK:
  // [Q row-major | dO row-major | Q^T]
  constexpr int IMGS = MODE == 0 ? 2 : 3;

  // one LDS object (a second __shared__ forces vmcnt(0) on every ds_read
  // — cdna guide §5 trap 4a).  lse/delta do NOT go through LDS: a
  // float-cast tail here defeated alias analysis and made hipcc emit
  // lgkmcnt(0) before EVERY ds_read of the stream images (50 full
  // drains per tile vs the dq kernel's counted waits — the round-2 wait
  // taxonomy's 58% parked dK).  They ride per-lane global loads,
  // prefetched one tile ahead, instead.
  __shared__ T lds[2 * IMGS * QBLK * D];
  auto ldsQ = [&](int buf) -> T* { return lds + buf * (IMGS * QBLK * D); };
  // MODE_DV: transposed dO; MODE_DK: row-major dO
  auto ldsG = [&](int buf) -> T* {
    return lds + buf * (IMGS * QBLK * D) + QBLK * D;
  };
  auto ldsQT = [&](int buf) -> T* {
    return lds + buf * (IMGS * QBLK * D) + 2 * QBLK * D;
  };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int n = blockIdx.y, b = blockIdx.z;
  const int kvb = blockIdx.x * 256 + wave * 32;
  const int kv_col = kvb + l31;

  // n is the kv head; the q-side pointers start at the group's first q
  // head (n itself without GQA) and step by one head stride per g
  const int n0 = GQA ? n * G : n;
  const int ng = GQA ? G : 1;
  const T* qp = q + b * q_sb + (int64_t)n0 * q_sh;
  const T* gp = dout + b * g_sb + (int64_t)n0 * g_sh;
  const float* dp_ = delta + b * d_sb + n0 * d_sh;
  const float* lp_ = lse + b * l_sb + n0 * l_sh;

  // resident K (always, for S); resident V when dP is needed
  frag kf[D / 16], vf[MODE == 1 ? D / 16 : 1];
  {
    const T* kp = k + b * k_sb + (int64_t)n * k_sh;
    const T* vp = v + b * v_sb + (int64_t)n * v_sh;
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      if (kv_col < Sk) {
        kf[s] = __builtin_bit_cast(
            frag,
            *(const u32x4_t*)(kp + (int64_t)kv_col * k_ss + 16 * s + 8 * hi));
        if (MODE == 1)
          vf[s] = __builtin_bit_cast(
              frag,
              *(const u32x4_t*)(vp + (int64_t)kv_col * v_ss + 16 * s + 8 * hi));
      } else {
        u32x4_t z = {0, 0, 0, 0};
        kf[s] = __builtin_bit_cast(frag, z);
        if (MODE == 1) vf[s] = __builtin_bit_cast(frag, z);
      }
    }
  }
  const float c2 = scale * BA_LOG2E;

  f32x16_t acc[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) acc[dt] = (f32x16_t)(0.f);

  // causal: q tiles wholly before this workgroup's kv rows are masked
  const int t0_shape = causal ? (blockIdx.x * 256) / QBLK : 0;
  const int nt_shape = (Sq + QBLK - 1) / QBLK;
  int2 trange = {t0_shape, nt_shape};
  int kid = 0, wk_min = 0, wk_max = 0;
  const int32_t* qseg = nullptr;
  const int2* tmm = nullptr;
  if constexpr (HAS_SEG) {
    const ba_seg_args sg = ba_seg_of(seg...);
    const int2 r = sg.blk_range[(int64_t)b * gridDim.x + blockIdx.x];
    trange.x = max(trange.x, r.x);
    trange.y = min(trange.y, r.y);
    if (trange.x >= trange.y) return;  // workgroup-uniform, no barrier yet
    kid = sg.kv_seg[b * sg.kv_sb + min(kv_col, Sk - 1)];
    ba_wave_minmax(kid, wk_min, wk_max);
    qseg = sg.q_seg + b * sg.q_sb;
    tmm = sg.tile_mm + (int64_t)b * ((Sq + QBLK - 1) / QBLK);
  }
  // band form: the block's q tile range is arithmetic; this kernel owns kv
  // rows, so it sees the band of (kv row - q row)
  ba_band_args bd = {0, 0};
  if constexpr (HAS_BAND) {
    bd = ba_band_flip(ba_band_of(seg...));
    const ba_tile_range r = ba_band_block_tiles(blockIdx.x, bd, Sk, Sq);
    trange.x = r.lo;
    trange.y = r.hi;
    if (trange.x >= trange.y) return;  // workgroup-uniform, no barrier yet
  }
  const int t0 = HAS_MASK ? trange.x : t0_shape;
  const int nt = HAS_MASK ? trange.y : nt_shape;

  // per-lane lse*log2e and delta for both subtiles of a tile (l2[qs] =
  // {lse2, delta}), loaded straight from global — clamped, branchless
  auto issue_loads = [&](int g, int tile, u32x4_t* qreg, u32x4_t* greg,
                         float2* l2) {
    const int q0 = tile * QBLK;
    const T* qpg = GQA ? qp + (int64_t)g * q_sh : qp;
    const T* gpg = GQA ? gp + (int64_t)g * g_sh : gp;
    const float* lpg = GQA ? lp_ + (int64_t)g * l_sh : lp_;
    const float* dpg = GQA ? dp_ + (int64_t)g * d_sh : dp_;
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      const int flat = tid + c * NT;
      const int row = flat / (D / 8), col8 = flat % (D / 8);
      // clamped instead of guarded (see attn_fwd.hip): out-of-range q
      // rows re-load row Sq-1; the q_g < Sq mask zeroes their P/dS, so
      // they contribute garbage x 0 to the dV/dK contractions
      const int qg = q0 + row;
      const int qc = qg < Sq ? qg : (Sq - 1);
      qreg[c] = *(const u32x4_t*)(qpg + (int64_t)qc * q_ss + col8 * 8);
      greg[c] = *(const u32x4_t*)(gpg + (int64_t)qc * g_ss + col8 * 8);
    }
#pragma unroll
    for (int qs = 0; qs < QBLK / 32; ++qs) {
      const int qg = q0 + qs * 32 + l31;
      const int qc = qg < Sq ? qg : (Sq - 1);
      // clamped rows contaminate nothing: the q_g < Sq mask zeroes p/dS
      l2[qs].x = lpg[qc] * BA_LOG2E;
      l2[qs].y = (MODE == 1) ? dpg[qc] : 0.f;
    }
  };
  auto write_lds = [&](int buf, const u32x4_t* qreg, const u32x4_t* greg) {
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      const int flat = tid + c * NT;
      const int row = flat / (D / 8), col8 = flat % (D / 8);
      const int byte = ba_swz<SWZ>(row * (2 * D) + col8 * 16, row);
      *(u32x4_t*)((char*)ldsQ(buf) + byte) = qreg[c];
      if (MODE == 0) {
        ba_st_transposed<T, QBLK, SWZ_T, 7>(ldsG(buf), row, col8 * 8, greg[c]);
      } else {
        // MODE_DK keeps the scatter-write transposed image: the tr16
        // address set spills ~47 VGPRs here (measured -14% fwd+bwd)
        *(u32x4_t*)((char*)ldsG(buf) + byte) = greg[c];
        ba_st_transposed<T, QBLK, SWZ_T, 7>(ldsQT(buf), row, col8 * 8, qreg[c]);
      }
    }
  };

  float2 l2c[QBLK / 32];
  {
    u32x4_t qreg[PT], greg[PT];
    issue_loads(0, t0, qreg, greg, l2c);
    write_lds(0, qreg, greg);
    __syncthreads();
  }
  if (__builtin_amdgcn_readfirstlane(threadIdx.x) >= 256)
    __builtin_amdgcn_s_setprio(1);  // T5 static form (younger half)

  // one flattened (g, tile) stream: the tile after a head's last one is
  // the next head's tile t0 (the causal t0 skip and the `active` test
  // depend on the tile index only, so they apply per head unchanged).
  // Without GQA ng == 1 folds this back to the single-head loop.
  int cur = 0;
  for (int g = 0; g < ng; ++g)
  for (int t = t0; t < nt; ++t) {
    const int q0 = t * QBLK;
    const bool last_t = (t + 1) >= nt;
    const bool has_next = !last_t || (GQA && g + 1 < ng);
    u32x4_t qreg[PT], greg[PT];
    float2 l2n[QBLK / 32] = {};
    if (has_next)
      issue_loads(last_t ? g + 1 : g, last_t ? t0 : t + 1, qreg, greg, l2n);

    bool active, seg_mask = false;
    if constexpr (HAS_SEG) {
      // segment form: the q tile's (min, max) ids against the wave's kv ids
      const int2 mm = tmm[t];
      seg_mask = !(mm.x == mm.y && wk_min == wk_max && mm.x == wk_min);
      active = (!causal || (q0 + QBLK - 1 >= kvb)) && mm.y >= wk_min &&
               mm.x <= wk_max;
    } else if constexpr (HAS_BAND) {
      active = ba_band_wave_active(kvb, q0, bd);
    } else {
      active = !causal || (q0 + QBLK - 1 >= kvb);
    }
    if (active) {
      const float2* ld2s = l2c;  // this tile's lse2/delta (prefetched)
#pragma unroll
      for (int qs = 0; qs < QBLK / 32; ++qs) {
        // ---- augmentation fold: the per-row constants ride the MFMA.
        // One extra k-slice per GEMM with B = [1,1,0...] (lanes of the
        // low half) and A carrying a row constant split hi/lo into two
        // fp16/bf16 elements (the split keeps the exponent-domain error
        // at fp32 roundoff): S accumulates -lse*log2e/c2 so the exp
        // argument is just st*c2; dP accumulates -delta so dS is just
        // p*dpt*scale.  Replaces 32 per-row LDS reads + fma/sub chains
        // (68% WAIT_ANY and 24 spilled VGPRs on the dK kernel).
        const float2 ld2 = ld2s[qs];
        frag ones01, ones0, a_lse, a_dlt;
        {
          u32x4_t z = {0, 0, 0, 0};
          ones01 = __builtin_bit_cast(frag, z);
          a_lse = __builtin_bit_cast(frag, z);
          a_dlt = __builtin_bit_cast(frag, z);
          if (hi == 0) {
            const float av = -ld2.x / c2;
            const T ah = (T)av;
            a_lse[0] = ah;
            a_lse[1] = (T)(av - (float)ah);
            const T dh = (T)(-ld2.y);
            a_dlt[0] = dh;
            a_dlt[1] = (T)(-ld2.y - (float)dh);
            ones01[0] = (T)1.f;
            ones01[1] = (T)1.f;
          }
          ones0 = ones01;
        }
        f32x16_t st = MT::mma(a_lse, ones01, (f32x16_t)(0.f));
        f32x16_t dpt = (f32x16_t)(0.f);
        if (MODE == 1) dpt = MT::mma(a_dlt, ones0, dpt);
#pragma unroll
        for (int s = 0; s < D / 16; ++s) {
          frag qfr = ba_ld_rowslice<T, D, SWZ>(ldsQ(cur), qs * 32 + l31,
                                               16 * s + 8 * hi);
          st = MT::mma(qfr, kf[s], st);
          if (MODE == 1) {
            frag gfr = ba_ld_rowslice<T, D, SWZ>(ldsG(cur), qs * 32 + l31,
                                                 16 * s + 8 * hi);
            dpt = MT::mma(gfr, vf[s], dpt);
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int q_loc = qs * 32 + ba_crow(r, 0) + 4 * hi;
          const int q_g = q0 + q_loc;
          bool valid =
              q_g < Sq && kv_col < Sk && (!causal || q_g >= kv_col);
          if constexpr (HAS_SEG)
            valid = valid && (!seg_mask || qseg[min(q_g, Sq - 1)] == kid);
          if constexpr (HAS_BAND)
            valid = valid && ba_band_visible(kv_col, q_g, bd);
          const float e = valid ? st[r] * c2 : BA_NEG_BIG;
          const float p = ba_exp2(e);
          // MODE_DV: P; MODE_DK: dS
          st[r] = (MODE == 0) ? p : p * dpt[r] * scale;
        }
        frag f01[2];
        ba_build_frag_pair<T>(st, f01);
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt) {
          const int drow = dt * 32 + l31;
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            // MODE_DV: A = dO^T row-slice; MODE_DK: A = Q^T row-slice
            const T* timg = (MODE == 0) ? ldsG(cur) : ldsQT(cur);
            frag tf = ba_ld_rowslice<T, QBLK, SWZ_T, 7>(
                timg, drow, qs * 32 + 16 * u + 8 * hi);
            acc[dt] = MT::mma(tf, f01[u], acc[dt]);
          }
        }
      }
    }
    if (has_next) write_lds(cur ^ 1, qreg, greg);
    __syncthreads();
    cur ^= 1;
#pragma unroll
    for (int qs = 0; qs < QBLK / 32; ++qs) l2c[qs] = l2n[qs];
  }

  if (kv_col < Sk) {
    // accumulate epilogue (single-writer per row: read-add-write)
    float* row = dout_acc + b * o_sb + (int64_t)kv_col * o_ss + n * o_sh;
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        row[dt * 32 + ba_crow(r, hi)] += acc[dt][r];
  }
}

// ============== fused dK + dQ kernel (kv-resident, flipped) ============
// FLIPPED orientation: S^T = mfma(K, Q) puts kv on the MFMA row axis and
// q on the lane axis, so lse/delta are LANE-LOCAL scalars (read straight
// from global, coalesced) — the split dK kernel's per-q-row constants
// (the "augmentation fold" MFMAs and their serial LDS->MFMA prologue,
// 65% SQ_WAIT in the round-1 PMCs) disappear.
//   dS^T sits in D-layout [kv rows][q cols].  From it:
//   * dQ fragments [row=q][contr=kv] come from ba_build_frag_pair
//     IN-REGISTER; dQ += mfma(dS^T, K^T) against a persistent K^T LDS
//     image (K is kv-block resident, staged transposed once).  Per-wave
//     partials (each wave owns 32 kv) are LDS-reduced (ds_add) across the
//     workgroup's 256 kv and flushed with ONE global fp32 atomic-add per
//     q-subtile — flash-attn's accumulation plan (hence deterministic=0
//     only).
//   * dK fragments [row=kv][contr=q] need the other orientation: a
//     per-wave LDS transpose (16 b16 scatter writes + 2 b128 reads, no
//     barrier — wave-private scratch); dK^T += mfma(Q^T, dS) stays
//     register-resident exactly like the split kernel.
// FUSE_DQ=0 degenerates to a flipped dK-only kernel (atomic-free — legal
// for deterministic=1; kept for A/B against the split MODE 1).
//
// Atomic-contention control: the grid is launched HEAD-FIRST
// (blockIdx.x = head) so concurrent workgroups flush different heads'
// dq regions, and non-causal workgroups start their q-tile stream at a
// per-kv-block offset (wrapping) so same-head workgroups flush
// DIFFERENT q tiles at any instant — without both, the 256 same-head
// workgroups march the same 16 KB of dq lines in lockstep and the
// line-serialised L2 RMWs dominate (measured 18x).
// DBG (env BA_DKQ_DBG, perf probes only — results wrong for >0):
//   1 = skip the global atomic flush;  2 = plain LDS writes, no ds_add;
//   3 = skip the whole dQ section (KT staging/LDS size/barriers kept);
//   4 = dQ MFMAs with dsT as both operands (no K^T LDS reads);
//   5 = dQ MFMAs + K^T reads, but no ds_add and no flush.
// SCRW: dS scratch row width (64 = conflict-free reads, 32 = half LDS).
//
// FUSE_DV=1 (requires FUSE_DQ=0): the 4-GEMM fused dK+dV kernel — adds
// P (kept beside dS), a streamed dO^T image, and a second accumulator:
//   dV^T? no — dV[kv][d] += mfma(P-frags [row=kv][contr=q],
//                                dO^T image [row=d][contr=q])
// P and dS share ONE per-wave scratch region sequentially (DS ops retire
// in order within a wave, so the write-read-write-read chain is safe
// without barriers).  This replaces BOTH split dkv kernels with 4 tile
// GEMMs instead of 5, atomic-free and deterministic — the measured
// verdict on gfx950 is that fp32 atomics (LDS ds_add ~2.6 s, global L2
// ~1.8 s at this density, each atomic dropping its L2 line) rule out
// flash-attn's atomic dq plan entirely (tools/dkq_probe.hip).
template <typename T, int D, int FUSE_DQ, int DBG = 0, int SCRW = 64,
          int FUSE_DV = 0>
__global__ __launch_bounds__(512) void bwd_dkq_kernel(
    const T* __restrict__ dout, const T* __restrict__ q,
    const T* __restrict__ k, const T* __restrict__ v,
    const float* __restrict__ delta, const float* __restrict__ lse,
    float* __restrict__ dq, float* __restrict__ dk, float* __restrict__ dv,
    int Sq, int Sk, int N,
    int64_t g_sb, int64_t g_ss, int64_t g_sh,
    int64_t q_sb, int64_t q_ss, int64_t q_sh,
    int64_t k_sb, int64_t k_ss, int64_t k_sh,
    int64_t v_sb, int64_t v_ss, int64_t v_sh,
    int64_t d_sb, int64_t d_sh, int64_t l_sb, int64_t l_sh,
    int64_t dq_sb, int64_t dq_ss, int64_t dq_sh,
    int64_t dk_sb, int64_t dk_ss, int64_t dk_sh,
    int64_t dv_sb, int64_t dv_ss, int64_t dv_sh,
    float scale, int causal) {
  static_assert(!(FUSE_DQ && FUSE_DV), "dq and dv fusions are exclusive");
  using MT = mfma_traits<T>;
  using frag = typename MT::frag;
  constexpr int QBLK = 32;    // streamed q rows per tile (1 subtile)
  constexpr int KVWG = 256;   // kv columns per workgroup (8 waves x 32)
  constexpr int NT = 512;
  constexpr int NIMG = 3 + FUSE_DV;         // Q, dO, Q^T [, dO^T]
  constexpr int SWZ = (D == 128) ? 15 : 7;  // Q/dO row-major images
  constexpr int SWZ_QT = 3;                 // Q^T image rows are 64 B
  constexpr int SWZ_SC = (SCRW == 64) ? 7 : 3;
  constexpr int CHUNKS = QBLK * (D / 8);    // staged 8-elem chunks per img

  // one LDS object (a second __shared__ forces vmcnt(0) per ds_read):
  // [2 buf x {Q row-major | dO row-major | Q^T | (dO^T)}] [K^T persistent]
  // [V row-major persistent (FUSE_DV — keeps the V fragments out of the
  // register file; kv-resident so staged once)] [8 x per-wave P/dS
  // scratch] [fp32 dq reduce buffer]
  constexpr int STREAM = 2 * NIMG * QBLK * D;
  constexpr int KT_E = FUSE_DQ ? D * KVWG : 0;
  constexpr int V_E = FUSE_DV ? D * KVWG : 0;
  constexpr int SCR_E = 8 * 32 * SCRW;
  constexpr int SCR2_E = FUSE_DV ? SCR_E : 0;  // separate P scratch
  constexpr int REDU_E = FUSE_DQ ? QBLK * D * (int)(4 / sizeof(T)) : 0;
  static_assert((STREAM + KT_E + V_E + SCR_E + SCR2_E + REDU_E) *
                        (int)sizeof(T) <=
                    163840,
                "LDS budget exceeded");
  __shared__ T lds[STREAM + KT_E + V_E + SCR_E + SCR2_E + REDU_E];
  auto ldsQ = [&](int buf) -> T* { return lds + buf * (NIMG * QBLK * D); };
  auto ldsG = [&](int buf) -> T* {
    return lds + buf * (NIMG * QBLK * D) + QBLK * D;
  };
  auto ldsQT = [&](int buf) -> T* {
    return lds + buf * (NIMG * QBLK * D) + 2 * QBLK * D;
  };
  auto ldsGT = [&](int buf) -> T* {  // FUSE_DV only
    return lds + buf * (NIMG * QBLK * D) + 3 * QBLK * D;
  };
  T* ldsKT = lds + STREAM;
  T* ldsV = lds + STREAM + KT_E;
  auto ldsSC = [&](int w) -> T* {
    return lds + STREAM + KT_E + V_E + w * 32 * SCRW;
  };
  auto ldsSC2 = [&](int w) -> T* {  // FUSE_DV: P scratch
    return lds + STREAM + KT_E + V_E + SCR_E + w * 32 * SCRW;
  };
  float* redu = (float*)(lds + STREAM + KT_E + V_E + SCR_E + SCR2_E);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int n = blockIdx.x, b = blockIdx.z;     // head-first dispatch
  const int kvblk = blockIdx.y;
  const int kvb = kvblk * KVWG + wave * 32;     // wave's kv block
  const int kv_col = kvb + l31;

  const T* qp = q + b * q_sb + (int64_t)n * q_sh;
  const T* gp = dout + b * g_sb + (int64_t)n * g_sh;
  const T* kp = k + b * k_sb + (int64_t)n * k_sh;
  const T* vp = v + b * v_sb + (int64_t)n * v_sh;
  const float* dp_ = delta + b * d_sb + n * d_sh;
  const float* lp_ = lse + b * l_sb + n * l_sh;

  // resident K fragments [row=kv][contr=d] (A operand of S^T); V the
  // same way in registers UNLESS FUSE_DV (register budget: it moves to
  // the persistent LDS image instead)
  frag kf[D / 16], vf[FUSE_DV ? 1 : D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    if (kv_col < Sk) {
      kf[s] = __builtin_bit_cast(
          frag, *(const u32x4_t*)(kp + (int64_t)kv_col * k_ss + 16 * s + 8 * hi));
      if (!FUSE_DV)
        vf[s] = __builtin_bit_cast(
            frag,
            *(const u32x4_t*)(vp + (int64_t)kv_col * v_ss + 16 * s + 8 * hi));
    } else {
      u32x4_t z = {0, 0, 0, 0};
      kf[s] = __builtin_bit_cast(frag, z);
      if (!FUSE_DV) vf[s] = __builtin_bit_cast(frag, z);
    }
  }
  const float c2 = scale * BA_LOG2E;

  f32x16_t acc[D / 32];  // dK^T accumulator [d rows][kv col = lane]
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) acc[dt] = (f32x16_t)(0.f);
  f32x16_t acc2[FUSE_DV ? D / 32 : 1];  // dV accumulator [kv rows][d col]
#pragma unroll
  for (int dt = 0; dt < (FUSE_DV ? D / 32 : 1); ++dt)
    acc2[dt] = (f32x16_t)(0.f);

  // one-time: zero the reduce buffer; stage K^T [D rows][KVWG] transposed
  if (FUSE_DQ) {
    for (int i = tid; i < QBLK * D; i += NT) redu[i] = 0.f;
    constexpr int PTK = (KVWG * D / 8) / NT;
#pragma unroll
    for (int c = 0; c < PTK; ++c) {
      const int flat = tid + c * NT;
      const int kv = flat / (D / 8), col8 = flat % (D / 8);
      const int kvg = kvblk * KVWG + kv;
      const int kvc = kvg < Sk ? kvg : (Sk - 1);
      u32x4_t ch = *(const u32x4_t*)(kp + (int64_t)kvc * k_ss + col8 * 8);
      ba_st_transposed<T, KVWG, 15, 0>(ldsKT, kv, col8 * 8, ch);
    }
  }
  // one-time (FUSE_DV): stage the workgroup's V block row-major
  if (FUSE_DV) {
    constexpr int PTV = (KVWG * D / 8) / NT;
#pragma unroll
    for (int c = 0; c < PTV; ++c) {
      const int flat = tid + c * NT;
      const int kv = flat / (D / 8), col8 = flat % (D / 8);
      const int kvg = kvblk * KVWG + kv;
      const int kvc = kvg < Sk ? kvg : (Sk - 1);
      u32x4_t ch = *(const u32x4_t*)(vp + (int64_t)kvc * v_ss + col8 * 8);
      const int byte = ba_swz<SWZ>(kv * (2 * D) + col8 * 16, kv);
      *(u32x4_t*)((char*)ldsV + byte) = ch;
    }
  }

  const int t0 = causal ? (kvblk * KVWG) / QBLK : 0;
  const int nt = (Sq + QBLK - 1) / QBLK;
  const int span = nt - t0;
  // non-causal stagger: spread same-head workgroups evenly over the
  // q-tile sequence (causal blocks are naturally staggered by t0)
  const int stag =
      (FUSE_DQ && !causal && gridDim.y > 1)
          ? (int)(((int64_t)kvblk * span) / gridDim.y)
          : 0;

  // per-tile prefetch: Q and dO chunks + this lane's lse*log2e and delta
  auto issue_loads = [&](int tile, u32x4_t* qreg, u32x4_t* greg, float* lse2,
                         float* dlt) {
    const int q0 = tile * QBLK;
    constexpr int PT = (CHUNKS + NT - 1) / NT;
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      const int flat = tid + c * NT;
      if (CHUNKS % NT == 0 || flat < CHUNKS) {
        const int row = flat / (D / 8), col8 = flat % (D / 8);
        const int qg = q0 + row;
        const int qc = qg < Sq ? qg : (Sq - 1);  // clamped (see attn_fwd.hip)
        qreg[c] = *(const u32x4_t*)(qp + (int64_t)qc * q_ss + col8 * 8);
        greg[c] = *(const u32x4_t*)(gp + (int64_t)qc * g_ss + col8 * 8);
      }
    }
    const int qg = q0 + l31;
    const int qc = qg < Sq ? qg : (Sq - 1);
    *lse2 = lp_[qc] * BA_LOG2E;  // lane-local; invalid rows masked later
    *dlt = dp_[qc];
  };
  auto write_lds = [&](int buf, const u32x4_t* qreg, const u32x4_t* greg) {
    constexpr int PT = (CHUNKS + NT - 1) / NT;
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      const int flat = tid + c * NT;
      if (CHUNKS % NT == 0 || flat < CHUNKS) {
        const int row = flat / (D / 8), col8 = flat % (D / 8);
        const int byte = ba_swz<SWZ>(row * (2 * D) + col8 * 16, row);
        *(u32x4_t*)((char*)ldsQ(buf) + byte) = qreg[c];
        *(u32x4_t*)((char*)ldsG(buf) + byte) = greg[c];
        ba_st_transposed<T, QBLK, SWZ_QT, 3>(ldsQT(buf), row, col8 * 8,
                                             qreg[c]);
        if (FUSE_DV)
          ba_st_transposed<T, QBLK, SWZ_QT, 3>(ldsGT(buf), row, col8 * 8,
                                               greg[c]);
      }
    }
  };

  float lse2_c, dlt_c;
  {
    u32x4_t qreg[(CHUNKS + NT - 1) / NT], greg[(CHUNKS + NT - 1) / NT];
    issue_loads(t0 + stag, qreg, greg, &lse2_c, &dlt_c);
    write_lds(0, qreg, greg);
    __syncthreads();
  }
  if (__builtin_amdgcn_readfirstlane(threadIdx.x) >= 256)
    __builtin_amdgcn_s_setprio(1);  // T5 static form (younger half)

  int cur = 0;
  int t = t0 + stag;  // wrapped iteration order over [t0, nt)
  for (int i = 0; i < span; ++i) {
    const int q0 = t * QBLK;
    int tn = t + 1;
    if (tn >= nt) tn = t0;
    const bool has_next = (i + 1) < span;
    u32x4_t qreg[(CHUNKS + NT - 1) / NT], greg[(CHUNKS + NT - 1) / NT];
    float lse2_n = 0.f, dlt_n = 0.f;
    if (has_next) issue_loads(tn, qreg, greg, &lse2_n, &dlt_n);

    // waves whose kv block is wholly after this q tile are masked anyway
    const bool active = !causal || (q0 + QBLK - 1 >= kvb);
    if (active) {
      // ---- S^T = mfma(K, Q), dP^T = mfma(V, dO): [kv rows][q cols]
      f32x16_t st = (f32x16_t)(0.f), dpt = (f32x16_t)(0.f);
#pragma unroll
      for (int s = 0; s < D / 16; ++s) {
        frag qfr = ba_ld_rowslice<T, D, SWZ>(ldsQ(cur), l31, 16 * s + 8 * hi);
        frag gfr = ba_ld_rowslice<T, D, SWZ>(ldsG(cur), l31, 16 * s + 8 * hi);
        frag vop;
        if (FUSE_DV)
          vop = ba_ld_rowslice<T, D, SWZ>(ldsV, wave * 32 + l31,
                                          16 * s + 8 * hi);
        else
          vop = vf[s];
        st = MT::mma(kf[s], qfr, st);
        dpt = MT::mma(vop, gfr, dpt);
      }
      // ---- dS^T = p * (dP^T - delta) * scale, lse/delta LANE-LOCAL.
      // FUSE_DV streams BOTH P and dS straight into their own per-wave
      // scratch regions inside this loop (no register homes, no
      // write-read-write serialisation): the dV/dK fragments read them
      // back transposed.
      T* sc = ldsSC(wave);
      T* sc2 = ldsSC2(wave);
      auto scr_byte = [&](int r) {
        const int row = ba_crow(r, 0) + 4 * hi;  // kv-local
        return ba_swz<SWZ_SC, 0>(row * (2 * SCRW) + 2 * l31, row);
      };
      const int q_g = q0 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kv_g = kvb + ba_crow(r, 0) + 4 * hi;
        const bool valid =
            q_g < Sq && kv_g < Sk && (!causal || q_g >= kv_g);
        const float e = valid ? __builtin_fmaf(st[r], c2, -lse2_c) : BA_NEG_BIG;
        const float p = ba_exp2(e);
        if (FUSE_DV) *(T*)((char*)sc2 + scr_byte(r)) = (T)p;
        st[r] = p * (dpt[r] - dlt_c) * scale;
      }
      auto scr_put = [&](const f32x16_t& vv) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          *(T*)((char*)sc + scr_byte(r)) = (T)vv[r];
      };
      // ---- per-wave scratch transpose: dS^T D-layout -> dS fragments
      // (own region — the dV section's P reads don't serialise against
      // these writes)
      scr_put(st);
      if (FUSE_DQ && DBG != 3) {
        // ---- dQ: fragments [row=q][contr=kv] in-register; one dt tile
        // at a time to keep the partial's register span at 16
        frag dsT[2];
        ba_build_frag_pair<T>(st, dsT);
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt) {
          f32x16_t dqp = (f32x16_t)(0.f);
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            frag ktf;
            if (DBG == 4)  // perf probe: no K^T LDS reads
              ktf = dsT[u];
            else
              ktf = ba_ld_rowslice<T, KVWG, 15, 0>(
                  ldsKT, dt * 32 + l31, wave * 32 + 16 * u + 8 * hi);
            dqp = MT::mma(dsT[u], ktf, dqp);
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int q_loc = ba_crow(r, 0) + 4 * hi;
            if (DBG == 5) {         // perf probe: no LDS reduce at all
              if (dqp[r] == 1234.5678f) redu[0] = dqp[r];  // keep dqp live
            } else if (DBG == 2)    // perf probe: write, not LDS-atomic
              redu[q_loc * D + dt * 32 + l31] = dqp[r];
            else
              atomicAdd(&redu[q_loc * D + dt * 32 + l31], dqp[r]);  // ds_add
          }
        }
      }
      if (FUSE_DV) {
        // ---- dV += mfma(P, dO^T): P read back from its own scratch
        frag pf[2];
        pf[0] = ba_ld_rowslice<T, SCRW, SWZ_SC, 0>(sc2, l31, 8 * hi);
        pf[1] = ba_ld_rowslice<T, SCRW, SWZ_SC, 0>(sc2, l31, 16 + 8 * hi);
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt) {
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            frag gt = ba_ld_rowslice<T, QBLK, SWZ_QT, 3>(
                ldsGT(cur), dt * 32 + l31, 16 * u + 8 * hi);
            acc2[dt] = MT::mma(pf[u], gt, acc2[dt]);
          }
        }
      }
      // ---- dK^T += mfma(Q^T, dS)
      frag dsf[2];
      dsf[0] = ba_ld_rowslice<T, SCRW, SWZ_SC, 0>(sc, l31, 8 * hi);
      dsf[1] = ba_ld_rowslice<T, SCRW, SWZ_SC, 0>(sc, l31, 16 + 8 * hi);
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          frag tf = ba_ld_rowslice<T, QBLK, SWZ_QT, 3>(
              ldsQT(cur), dt * 32 + l31, 16 * u + 8 * hi);
          acc[dt] = MT::mma(tf, dsf[u], acc[dt]);
        }
      }
    }
    if (!FUSE_DQ) {
      if (has_next) write_lds(cur ^ 1, qreg, greg);
      __syncthreads();
    } else {
      __syncthreads();  // A: every wave's ds_adds for this tile landed
      // flush the reduced dq partial: ONE atomic per element per
      // workgroup (the ds_adds above summed the 8 waves' 32-kv
      // partials).  Issued BEFORE write_lds so the staging's counted
      // vmcnt wait does not drain the fire-and-forget atomics.
      const int base = tid * (QBLK * D / NT);  // 8 consecutive floats
      const int q_loc = base / D, d0 = base % D;
      const int q_g2 = q0 + q_loc;
      if (q_g2 < Sq && DBG != 1 && DBG != 5) {
        float* gdst = dq + b * dq_sb + (int64_t)q_g2 * dq_ss + n * dq_sh + d0;
#pragma unroll
        for (int j = 0; j < QBLK * D / NT; ++j) {
          unsafeAtomicAdd(&gdst[j], redu[base + j]);
          redu[base + j] = 0.f;
        }
      } else {
#pragma unroll
        for (int j = 0; j < QBLK * D / NT; ++j) redu[base + j] = 0.f;
      }
      if (has_next) write_lds(cur ^ 1, qreg, greg);
      __syncthreads();  // B: redu zeroed + staging visible
    }
    cur ^= 1;
    lse2_c = lse2_n;
    dlt_c = dlt_n;
    t = tn;
  }

  if (kv_col < Sk) {
    float* row = dk + b * dk_sb + (int64_t)kv_col * dk_ss + n * dk_sh;
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        row[dt * 32 + ba_crow(r, hi)] += acc[dt][r];
  }
  if (FUSE_DV) {
    // dV accumulator sits [kv rows][d col = lane]: per (r, dt) the 32
    // lanes of a half write one kv row's 128 B contiguously
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kv_g = kvb + ba_crow(r, 0) + 4 * hi;
      if (kv_g < Sk) {
        float* row2 = dv + b * dv_sb + (int64_t)kv_g * dv_ss + n * dv_sh;
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt)
          row2[dt * 32 + l31] += acc2[dt][r];
      }
    }
  }
}

}  // namespace

// ====================== launchers =====================================
extern "C" int bahip_attn_bwd_preprocess(
    const void* o, const void* dout, float* delta, int64_t B, int64_t S,
    int64_t N, int64_t D, const int64_t o_strides[3],
    const int64_t do_strides[3], int o_dtype, int do_dtype, void* stream) {
  if (o_dtype != do_dtype)
    return ba_fail(BAHIP_ERR_DTYPE_MISMATCH,
                   "o / dout dtype mismatch (%d vs %d)", o_dtype, do_dtype);
  dim3 grid((unsigned)((S + 31) / 32), (unsigned)N, (unsigned)B);
  return ba_dispatch_td(D, o_dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    bwd_preprocess_kernel<T, decltype(td)::D>
        <<<grid, 256, 0, (hipStream_t)stream>>>(
            (const T*)o, (const T*)dout, delta, (int)S, (int)N, o_strides[0],
            o_strides[1], o_strides[2], do_strides[0], do_strides[1],
            do_strides[2]);
    return ba_launch_status();
  });
}

// ---- backward launch layer --------------------------------------------
// Which kernels a knob combination launches: ba_bwd_select, bwd_plans.h;
// what was measured for each plan: DESIGN.md.  All plans accumulate into
// dq/dk/dv; split8 and dkvf7 are bitwise deterministic (the
// `deterministic` flag is honoured by construction).
//
// One field per kernel parameter, in kernel order; the launch templates
// expand a struct into the <<<>>> call and derive the grid, and
// tools/dkq_probe.hip launches through the same pairs.  bwd_dq_kernel and
// bwd_dkv_kernel take the same list — the inputs, one fp32 accumulator
// (dq; dv for MODE 0, dk for MODE 1) and its strides — so they share one.
struct bwd_dq_args {
  const void *dout, *q, *k, *v;
  const float *delta, *lse;
  float* out;
  int Sq, Sk, N, G;
  int64_t g_sb, g_ss, g_sh, q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, v_sb, v_ss,
      v_sh, d_sb, d_sh, l_sb, l_sh, o_sb, o_ss, o_sh;
  float scale;
  int causal;
};
using bwd_dkv_args = bwd_dq_args;
using bwd_dq_kernel_t = decltype(&bwd_dq_kernel<_Float16, 128, 0>);
static_assert(
    std::is_same_v<bwd_dq_kernel_t,
                   decltype(&bwd_dkv_kernel<_Float16, 128, 0, 64, 0>)> &&
        sizeof(bwd_dq_args) == kernarg_size<bwd_dq_kernel_t>::value,
    "bwd_dq_args must mirror bwd_dq_kernel's and bwd_dkv_kernel's parameters");

// `seg`: nothing, or the ba_seg_args of a segment-form kernel
template <typename T, typename K, typename... SEG>
static void launch_acc(K kernel, dim3 grid, const bwd_dq_args& a,
                       hipStream_t stream, SEG... seg) {
  kernel<<<grid, 512, 0, stream>>>(
      (const T*)a.dout, (const T*)a.q, (const T*)a.k, (const T*)a.v, a.delta,
      a.lse, a.out, a.Sq, a.Sk, a.N, a.G, a.g_sb, a.g_ss, a.g_sh, a.q_sb,
      a.q_ss, a.q_sh, a.k_sb, a.k_ss, a.k_sh, a.v_sb, a.v_ss, a.v_sh, a.d_sb,
      a.d_sh, a.l_sb, a.l_sh, a.o_sb, a.o_ss, a.o_sh, a.scale, a.causal,
      seg...);
}

template <typename T, int D, int DQP>
static void launch_dq(const bwd_dq_args& a, int64_t B, hipStream_t stream) {
  const dim3 grid((unsigned)((a.Sq + 255) / 256), (unsigned)a.N, (unsigned)B);
  launch_acc<T>(bwd_dq_kernel<T, D, DQP>, grid, a, stream);
}

// one workgroup column per KV head; G > 1 runs the group-loop (GQA = 1) form
template <typename T, int D, int MODE>
static void launch_dkv(const bwd_dkv_args& a, int64_t B, hipStream_t stream) {
  const dim3 grid((unsigned)((a.Sk + 255) / 256), (unsigned)(a.N / a.G),
                  (unsigned)B);
  launch_acc<T>(a.G > 1 ? bwd_dkv_kernel<T, D, MODE, 64, 1>
                        : bwd_dkv_kernel<T, D, MODE, 64, 0>,
                grid, a, stream);
}

// the segment forms of the default plan's three kernels; the two sides'
// pre-pass regions differ (dq owns q rows, dK/dV own kv rows)
template <typename T, int D>
static void launch_dq_seg(const bwd_dq_args& a, const ba_seg_args& sg,
                          int64_t B, hipStream_t stream) {
  const dim3 grid((unsigned)((a.Sq + 255) / 256), (unsigned)a.N, (unsigned)B);
  launch_acc<T>(bwd_dq_kernel<T, D, 0, ba_seg_args>, grid, a, stream, sg);
}
template <typename T, int D, int MODE>
static void launch_dkv_seg(const bwd_dkv_args& a, const ba_seg_args& sg,
                           int64_t B, hipStream_t stream) {
  const dim3 grid((unsigned)((a.Sk + 255) / 256), (unsigned)(a.N / a.G),
                  (unsigned)B);
  if (a.G > 1)
    launch_acc<T>(bwd_dkv_kernel<T, D, MODE, 64, 1, ba_seg_args>, grid, a,
                  stream, sg);
  else
    launch_acc<T>(bwd_dkv_kernel<T, D, MODE, 64, 0, ba_seg_args>, grid, a,
                  stream, sg);
}

// the band forms of the same three kernels: no pre-pass, the band itself
template <typename T, int D>
static void launch_dq_band(const bwd_dq_args& a, const ba_band_args& bd,
                           int64_t B, hipStream_t stream) {
  const dim3 grid((unsigned)((a.Sq + 255) / 256), (unsigned)a.N, (unsigned)B);
  launch_acc<T>(bwd_dq_kernel<T, D, 0, ba_band_args>, grid, a, stream, bd);
}
template <typename T, int D, int MODE>
static void launch_dkv_band(const bwd_dkv_args& a, const ba_band_args& bd,
                            int64_t B, hipStream_t stream) {
  const dim3 grid((unsigned)((a.Sk + 255) / 256), (unsigned)(a.N / a.G),
                  (unsigned)B);
  if (a.G > 1)
    launch_acc<T>(bwd_dkv_kernel<T, D, MODE, 64, 1, ba_band_args>, grid, a,
                  stream, bd);
  else
    launch_acc<T>(bwd_dkv_kernel<T, D, MODE, 64, 0, ba_band_args>, grid, a,
                  stream, bd);
}

struct bwd_dkq_args {
  const void *dout, *q, *k, *v;
  const float *delta, *lse;
  float *dq, *dk, *dv;
  int Sq, Sk, N;
  int64_t g_sb, g_ss, g_sh, q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, v_sb, v_ss,
      v_sh, d_sb, d_sh, l_sb, l_sh, dq_sb, dq_ss, dq_sh, dk_sb, dk_ss, dk_sh,
      dv_sb, dv_ss, dv_sh;
  float scale;
  int causal;
};
static_assert(sizeof(bwd_dkq_args) ==
                  kernarg_size<decltype(&bwd_dkq_kernel<_Float16, 128, 0>)>::value,
              "bwd_dkq_args must mirror bwd_dkq_kernel's parameter list");

// head-first grid (see the atomic-contention note above bwd_dkq_kernel)
template <typename T, int D, int FUSE_DQ, int DBG = 0, int SCRW = 64,
          int FUSE_DV = 0>
static void launch_dkq(const bwd_dkq_args& a, int64_t B, hipStream_t stream) {
  const dim3 grid((unsigned)a.N, (unsigned)((a.Sk + 255) / 256), (unsigned)B);
  bwd_dkq_kernel<T, D, FUSE_DQ, DBG, SCRW, FUSE_DV><<<grid, 512, 0, stream>>>(
      (const T*)a.dout, (const T*)a.q, (const T*)a.k, (const T*)a.v, a.delta,
      a.lse, a.dq, a.dk, a.dv, a.Sq, a.Sk, a.N, a.g_sb, a.g_ss, a.g_sh, a.q_sb,
      a.q_ss, a.q_sh, a.k_sb, a.k_ss, a.k_sh, a.v_sb, a.v_ss, a.v_sh, a.d_sb,
      a.d_sh, a.l_sb, a.l_sh, a.dq_sb, a.dq_ss, a.dq_sh, a.dk_sb, a.dk_ss,
      a.dk_sh, a.dv_sb, a.dv_ss, a.dv_sh, a.scale, a.causal);
}

// what bahip_attn_bwd_seg adds to the plain call
struct bwd_seg_call {
  const int32_t *q_seg, *kv_seg;
  int64_t q_sb, kv_sb;
  void* ws;
  int64_t ws_bytes;
};

// what bahip_attn_bwd_band adds to the plain call: the band as given
struct bwd_band_call {
  int64_t lo, hi;
};

// Shared body of the backward entry points; seg and band null = the plain
// call.
static int bwd_entry(
    const void* dout, const void* q, const void* k, const void* v,
    const float* delta, const float* lse, float* dq, float* dk, float* dv,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t gs[3], const int64_t qs[3], const int64_t ks[3],
    const int64_t vs[3], const int64_t ds[2], const int64_t ls[2],
    const int64_t dqs[3], const int64_t dks[3], const int64_t dvs[3],
    float scale, int causal, int deterministic, int dtype, void* stream,
    const bwd_seg_call* seg, const bwd_band_call* band = nullptr) {
  (void)deterministic;  // only atomic6 is not deterministic by construction
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
  // read per call (cheap at one bwd invocation) so tests can flip plans
  ba_bwd_knobs kn;
  kn.fused = ba_env_int(BA_BWD_KNOB_SPECS[0].env, kn.fused);
  kn.dk_flip = ba_env_int(BA_BWD_KNOB_SPECS[1].env, kn.dk_flip);
  kn.dq_pipe = ba_env_int(BA_BWD_KNOB_SPECS[2].env, kn.dq_pipe);
  kn.dkq_dbg = ba_env_int(BA_BWD_KNOB_SPECS[3].env, kn.dkq_dbg);
  const ba_bwd_plan plan = ba_bwd_select(kn, G);
  if (plan.verdict == BA_BWD_BAD_VALUE)
    return ba_fail(BAHIP_ERR_BAD_KNOB, "%s=%d is not an accepted value",
                   plan.knob, plan.value);
  if (plan.verdict == BA_BWD_NO_GQA)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "%s=%d does not support grouped-query heads "
                   "(N=%d, Nk=%d)",
                   plan.knob, plan.value, (int)N, (int)Nk);
  const int iSq = (int)Sq, iSk = (int)Sk, iN = (int)N;
  const auto acc_into = [&](float* out, const int64_t* os) -> bwd_dq_args {
    return {dout, q, k, v, delta, lse, out, iSq, iSk, iN, G,
            gs[0], gs[1], gs[2], qs[0], qs[1], qs[2], ks[0], ks[1], ks[2],
            vs[0], vs[1], vs[2], ds[0], ds[1], ls[0], ls[1],
            os[0], os[1], os[2], scale, causal};
  };
  const bwd_dq_args dqa = acc_into(dq, dqs);
  const bwd_dkv_args dva = acc_into(dv, dvs), dka = acc_into(dk, dks);
  if (seg) {
    // the default plan's kernels in their segment form, after the pre-pass
    // of both side pairs, all on `stream`
    const ba_seg_verdict sv = ba_seg_bwd_support(kn);
    if (sv.knob)
      return ba_fail(BAHIP_ERR_UNSUPPORTED,
                     "%s=%d does not support segment ids (default backward "
                     "plan only)",
                     sv.knob, sv.value);
    if (B < 1 || B > 65535 || Sq < 1 || Sk < 1)
      return ba_fail(BAHIP_ERR_UNSUPPORTED,
                     "segment ids: unsupported shape B=%d Sq=%d Sk=%d", (int)B,
                     (int)Sq, (int)Sk);
    if (!seg->ws || seg->ws_bytes < ba_seg_ws_bytes(B, Sq, Sk))
      return ba_fail(BAHIP_ERR_WORKSPACE,
                     "segment workspace of %lld bytes is smaller than the "
                     "%lld needed",
                     (long long)(seg->ws ? seg->ws_bytes : 0),
                     (long long)ba_seg_ws_bytes(B, Sq, Sk));
    const ba_seg_ws_layout w = ba_seg_ws(B, Sq, Sk);
    int32_t* ws = (int32_t*)seg->ws;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = bahip_attn_seg_prepass(seg->q_seg, seg->kv_seg, seg->q_sb,
                                        seg->kv_sb, B, Sq, Sk, seg->ws,
                                        seg->ws_bytes, stream))
      return rc;
    const ba_seg_args own_q = {seg->q_seg, seg->kv_seg, seg->q_sb, seg->kv_sb,
                               (const int2*)(ws + w.kv_tile_mm),
                               (const int2*)(ws + w.q_blk_range)};
    const ba_seg_args own_kv = {seg->q_seg, seg->kv_seg, seg->q_sb, seg->kv_sb,
                                (const int2*)(ws + w.q_tile_mm),
                                (const int2*)(ws + w.kv_blk_range)};
    return ba_dispatch_td(D, dtype, [&](auto td) {
      using T = typename decltype(td)::type;
      constexpr int TD = decltype(td)::D;
      launch_dq_seg<T, TD>(dqa, own_q, B, st);
      BA_CHECK_LAUNCH();
      launch_dkv_seg<T, TD, 0>(dva, own_kv, B, st);
      BA_CHECK_LAUNCH();
      launch_dkv_seg<T, TD, 1>(dka, own_kv, B, st);
      return ba_launch_status();
    });
  }
  if (band) {
    // the default plan's kernels in their band form
    if (band->lo > band->hi)
      return ba_fail(BAHIP_ERR_BAND, "band: lo=%lld is above hi=%lld",
                     (long long)band->lo, (long long)band->hi);
    const ba_seg_verdict sv = ba_seg_bwd_support(kn);
    if (sv.knob)
      return ba_fail(BAHIP_ERR_UNSUPPORTED,
                     "%s=%d does not support a band (default backward plan "
                     "only)",
                     sv.knob, sv.value);
    if (B < 1 || B > 65535 || Sq < 1 || Sk < 1)
      return ba_fail(BAHIP_ERR_UNSUPPORTED,
                     "band: unsupported shape B=%d Sq=%d Sk=%d", (int)B,
                     (int)Sq, (int)Sk);
    // causal cuts the band at the diagonal: the band kernels never read
    // `causal`
    const ba_band_args bd = {
        ba_band_clamp(causal && band->lo < 0 ? 0 : band->lo),
        ba_band_clamp(band->hi)};
    const hipStream_t st = (hipStream_t)stream;
    return ba_dispatch_td(D, dtype, [&](auto td) {
      using T = typename decltype(td)::type;
      constexpr int TD = decltype(td)::D;
      launch_dq_band<T, TD>(dqa, bd, B, st);
      BA_CHECK_LAUNCH();
      launch_dkv_band<T, TD, 0>(dva, bd, B, st);
      BA_CHECK_LAUNCH();
      launch_dkv_band<T, TD, 1>(dka, bd, B, st);
      return ba_launch_status();
    });
  }
  const bwd_dkq_args dkqa = {
      dout, q, k, v, delta, lse, dq, dk, dv, iSq, iSk, iN,
      gs[0], gs[1], gs[2], qs[0], qs[1], qs[2], ks[0], ks[1], ks[2],
      vs[0], vs[1], vs[2], ds[0], ds[1], ls[0], ls[1],
      dqs[0], dqs[1], dqs[2], dks[0], dks[1], dks[2],
      dvs[0], dvs[1], dvs[2], scale, causal};
  return ba_dispatch_td(D, dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    constexpr int TD = decltype(td)::D;
    const hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < plan.n_steps; ++i) {
      switch (plan.steps[i]) {
        case BA_STEP_DQ: launch_dq<T, TD, 0>(dqa, B, st); break;
        case BA_STEP_DQ_PIPE: launch_dq<T, TD, 1>(dqa, B, st); break;
        case BA_STEP_DV: launch_dkv<T, TD, 0>(dva, B, st); break;
        case BA_STEP_DK: launch_dkv<T, TD, 1>(dka, B, st); break;
        case BA_STEP_DK_FLIPPED: launch_dkq<T, TD, 0>(dkqa, B, st); break;
        case BA_STEP_DKDV_FUSED: launch_dkq<T, TD, 0, 0, 32, 1>(dkqa, B, st); break;
        case BA_STEP_DKDQ_ATOMIC: launch_dkq<T, TD, 1, 0>(dkqa, B, st); break;
        case BA_STEP_DKDQ_DBG1: launch_dkq<T, TD, 1, 1>(dkqa, B, st); break;
        case BA_STEP_DKDQ_DBG2: launch_dkq<T, TD, 1, 2>(dkqa, B, st); break;
      }
      BA_CHECK_LAUNCH();
    }
    return 0;
  });
}

extern "C" int bahip_attn_bwd_gqa(
    const void* dout, const void* q, const void* k, const void* v,
    const float* delta, const float* lse, float* dq, float* dk, float* dv,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t gs[3], const int64_t qs[3], const int64_t ks[3],
    const int64_t vs[3], const int64_t ds[2], const int64_t ls[2],
    const int64_t dqs[3], const int64_t dks[3], const int64_t dvs[3],
    float scale, int causal, int deterministic, int dtype, void* stream) {
  return bwd_entry(dout, q, k, v, delta, lse, dq, dk, dv, B, Sq, Sk, N, Nk, D,
                   gs, qs, ks, vs, ds, ls, dqs, dks, dvs, scale, causal,
                   deterministic, dtype, stream, nullptr);
}

extern "C" int bahip_attn_bwd_seg(
    const void* dout, const void* q, const void* k, const void* v,
    const float* delta, const float* lse, float* dq, float* dk, float* dv,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t gs[3], const int64_t qs[3], const int64_t ks[3],
    const int64_t vs[3], const int64_t ds[2], const int64_t ls[2],
    const int64_t dqs[3], const int64_t dks[3], const int64_t dvs[3],
    float scale, int causal, int deterministic, int dtype,
    const int32_t* q_seg, const int32_t* kv_seg, int64_t q_seg_stride,
    int64_t kv_seg_stride, void* seg_workspace, int64_t seg_workspace_bytes,
    void* stream) {
  if ((q_seg == nullptr) != (kv_seg == nullptr))
    return ba_fail(BAHIP_ERR_SEGMENT_IDS,
                   "segment ids: q_seg and kv_seg must both be given or both "
                   "be null (%s is null)",
                   q_seg ? "kv_seg" : "q_seg");
  const bwd_seg_call sc = {q_seg, kv_seg, q_seg_stride, kv_seg_stride,
                           seg_workspace, seg_workspace_bytes};
  return bwd_entry(dout, q, k, v, delta, lse, dq, dk, dv, B, Sq, Sk, N, Nk, D,
                   gs, qs, ks, vs, ds, ls, dqs, dks, dvs, scale, causal,
                   deterministic, dtype, stream, q_seg ? &sc : nullptr);
}

extern "C" int bahip_attn_bwd_band(
    const void* dout, const void* q, const void* k, const void* v,
    const float* delta, const float* lse, float* dq, float* dk, float* dv,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t gs[3], const int64_t qs[3], const int64_t ks[3],
    const int64_t vs[3], const int64_t ds[2], const int64_t ls[2],
    const int64_t dqs[3], const int64_t dks[3], const int64_t dvs[3],
    float scale, int causal, int deterministic, int dtype, int64_t band_lo,
    int64_t band_hi, void* stream) {
  const bwd_band_call bc = {band_lo, band_hi};
  return bwd_entry(dout, q, k, v, delta, lse, dq, dk, dv, B, Sq, Sk, N, Nk, D,
                   gs, qs, ks, vs, ds, ls, dqs, dks, dvs, scale, causal,
                   deterministic, dtype, stream, nullptr, &bc);
}

// the equal-heads symbol: Nk = N
extern "C" int bahip_attn_bwd(
    const void* dout, const void* q, const void* k, const void* v,
    const float* delta, const float* lse, float* dq, float* dk, float* dv,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t D,
    const int64_t do_strides[3], const int64_t q_strides[3],
    const int64_t k_strides[3], const int64_t v_strides[3],
    const int64_t delta_strides[2], const int64_t lse_strides[2],
    const int64_t dq_strides[3], const int64_t dk_strides[3],
    const int64_t dv_strides[3], float softmax_scale, int causal,
    int deterministic, int dtype, void* stream) {
  return bahip_attn_bwd_gqa(dout, q, k, v, delta, lse, dq, dk, dv, B, Sq, Sk,
                            N, N, D, do_strides, q_strides, k_strides,
                            v_strides, delta_strides, lse_strides, dq_strides,
                            dk_strides, dv_strides, softmax_scale, causal,
                            deterministic, dtype, stream);
}
