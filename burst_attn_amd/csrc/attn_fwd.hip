// BurstAttention forward tile kernel for gfx950 (MI355X, CDNA4).
//
// Computes one flash-attention tile o = softmax(q k^T * scale) v plus its
// log-sum-exp — the role the flash-attn CUDA extension plays for the
// reference at burst_attn/burst_utils.py:149-177 — as a single hand-written
// HIP kernel (online softmax in the exp2 domain, fused, no S matrix in HBM).
//
// Structure (see attn_common.h header comment for the operand scheme):
//   * workgroup = 8 waves (512 threads); wave w owns q rows
//     [blk*256 + w*32, +32); grid = (ceil(Sq/256), N, B).
//   * kv tiles of KVBLK=64 rows staged in LDS, double-buffered, one barrier
//     per tile; next tile's global loads are issued before the current
//     tile's MFMAs (async-stage split).  K is stored row-major [kv][D]
//     (XOR-swizzled); V is stored TRANSPOSED [D][kv] at staging time so
//     that both operands' MFMA fragments are plain 16B row-slice
//     ds_read_b128s — no per-element transposed gathers (those made the
//     compiler hoist & spill hundreds of swizzled addresses).  With a
//     workspace the transpose is done once per call by
//     attn_vt_image_kernel instead and the default variant's VSRC=1 form
//     copies V^T tiles as it copies K (vt_image.h).
//   * per kv tile and wave: S^T = mfma(K, Q) (2 x D/16 MFMAs),
//     online-softmax update (lane-local m/l in exp2 domain),
//     P->fragments in-register (pack + permlane32_swap),
//     O^T += mfma(V^T, P^T) (2 x 2 x D/32 MFMAs).
//   * epilogue: o = O^T / l (fp32 out), lse = ln2*(m2 + log2(l)).

#include "attn_common.h"
#include "attn_host.h"
#include "fwd_variants.h"
#include "gqa_heads.h"
#include "seg_support.h"
#include "vt_image.h"

#include <stddef.h>

namespace {

// Buffer index of one tile-loop copy: a compile-time literal (ba_ic) in the
// loop unrolled by the buffer period, a runtime value (ba_dyn) in the rolled
// one.
template <int N>
struct ba_ic {
  static constexpr int value = N;
};
struct ba_dyn {
  int value;
};
template <int N>
__device__ __forceinline__ int ba_buf_of(ba_ic<N>) { return N; }
__device__ __forceinline__ int ba_buf_of(ba_dyn d) { return d.value; }

// OUT_STATE=0: write normalised o (fp32) + lse — the stateless tile.
// OUT_STATE=1: carry-in/carry-out accumulator state (acc = unnormalised
// O, m = running max in the exp2 domain, l = running sum) — the fused
// in-kernel merge replacing the reference's per-round
// cuda_scale_out_lse_helper pass (burst_utils.py:20-33; lao.py's
// carry-in design, lao.py:108-114).
// VPATH: 0 = V transposed image + b128 row-slice reads;
//         1 = V row-major (tr16-swizzled) + ds_read_tr16_b64 fragments
// SUBT: 0 = joint softmax over the 64-kv tile; 1 = per-32-subtile online
// updates (lets subtile-0 PV MFMAs overlap subtile-1 QK/softmax);
// 2 = att[2] double-pipeline (guide T15): the softmax FINISH (mask, max,
// rescale, exp2, pack) and PV of subtile j-1 are issued while subtile
// j's QK MFMAs fill — an explicit two-stage software pipeline carried
// ACROSS tile boundaries (requires NBUF=4 so the previous tile's V
// image survives one extra subtile, and a barrier every tile);
// 3 = THREE-stage pipeline at ONE WAVE PER SIMD (worksheet-driven,
// profiles/r02/mfma_pipe_worksheet.txt): phase k issues QK(k) MFMAs,
// the softmax of subtile k-1 (producing the P fragments), and PV(k-2)
// — three independent chains per wave, K/V fragments prefetched a full
// phase ahead into registers.  Requires NT=256 and NBUF=4 (128 KB LDS
// forces one 4-wave workgroup per CU = 1 wave/SIMD, where the ~500
// register budget holds the pipeline state).  The ot rescale of
// softmax(k-1) is ordered AFTER PV(k-2) lands (scale consistency).
// NT: threads per workgroup (512 = 8 waves x 1 block/CU;
//     256 = 4 waves x 2 blocks/CU — decoupled barrier groups)
// NBUF: LDS tile buffers. 2 = stage one tile ahead, barrier every tile.
// 4 = stage two tiles ahead, barrier every OTHER tile (a buffer is
// rewritten two tiles after its last read, so one barrier in any two
// consecutive tile boundaries separates every write from its readers
// and every reader from the overwrite).
// KREG: 1 = K tiles go straight from HBM into the MFMA fragment
// registers (no LDS round trip): the QK cluster is PURE-REG (guide T16's
// load-K->reg cluster), and tile t+1's K loads are issued the moment
// tile t's QK MFMAs consume the block (WAR on the same registers), so
// softmax+PV+staging+barrier (~700+ cycles) cover the HBM latency.
// Only the V^T image stays in LDS.  Requires SUBT=1, NBUF=2, VPATH=0.
// (Measured -47%: the per-lane strided K loads swamp vmem issue.)
// KREG=2 = cross-barrier K-FRAGMENT PREFETCH: one 8-fragment register
// set is re-filled from LDS a full SUBTILE ahead of its QK use — legal
// across tile boundaries because NBUF=4 staging (AHEAD=2) wrote tile
// t+1's buffer two tiles ago and a barrier every tile orders it.  The
// QK cluster's lgkm park (SQ_WAIT_ANY 38% in the r2 PMC taxonomy)
// becomes overlap.  Requires SUBT=1, NBUF=4, VPATH=0.
// VSRC: where the V^T LDS image comes from.  0 = V itself, transposed at
// staging time (16 two-byte LDS writes per thread and tile at D=128);
// 1 = the V^T image of vt_image.h, written once per call by
// attn_vt_image_kernel: `v` points at the image, v_sb / v_sh are its batch
// and head strides, v_ss is unused, and a tile's staging is PT 16-byte
// copies like K's.  Default variant <0,1,512,2,0> only.
// SEG: empty = the plain kernel.  One ba_seg_args = the segment-id form
// (attn_common.h): the id equality joins the boundary mask; the tile loop
// covers only the block's [lo, hi) range from the pre-pass; a wave skips a
// tile whose (min, max) ids miss those of its rows; masked entries get
// weight exactly 0, so a row that sees no key ends with l = 0; a workgroup
// with an empty range leaves before its first barrier.  Default variant
// with VSRC=0 only.
template <typename T, int D, int KVBLK, int OUT_STATE, int VPATH, int SUBT,
          int NT = 512, int NBUF = 2, int KREG = 0, int VSRC = 0,
          typename... SEG>
__global__ __launch_bounds__(NT) void attn_fwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
    float* __restrict__ o, float* __restrict__ lse,
    int Sq, int Sk, int N, int G,
    int64_t q_sb, int64_t q_ss, int64_t q_sh,
    int64_t k_sb, int64_t k_ss, int64_t k_sh,
    int64_t v_sb, int64_t v_ss, int64_t v_sh,
    float scale, int causal,
    // state (OUT_STATE=1): acc [B,Sq,N,D] strided, m/l [B,N,Sq] strided
    float* __restrict__ st_acc, float* __restrict__ st_m,
    float* __restrict__ st_l,
    int64_t a_sb, int64_t a_ss, int64_t a_sh,
    int64_t ml_sb, int64_t ml_sh, int carry_in, SEG... seg) {
  using MT = mfma_traits<T>;
  using frag = typename MT::frag;
  constexpr bool HAS_BAND = ba_pack_is<ba_band_args, SEG...>;
  constexpr bool HAS_SEG = sizeof...(SEG) != 0 && !HAS_BAND;
  // either form: entries can be masked inside the tensors' ranges, so a row
  // may see no key (weight-0 select, l = 0 epilogue)
  constexpr bool HAS_MASK = HAS_SEG || HAS_BAND;
  static_assert(!HAS_MASK || (sizeof...(SEG) == 1 && VPATH == 0 && SUBT == 1 &&
                              NT == 512 && NBUF == 2 && KREG == 0 && VSRC == 0),
                "segment ids / band: the default variant, V transposed "
                "in-kernel");
  static_assert(!HAS_BAND || (KVBLK == BA_BAND_TILE && NT / 2 == BA_BAND_BLOCK),
                "band: the tile sizes of band_support.h");
  // band form: the band is the whole mask (the launcher folded causal in)
  if constexpr (HAS_BAND) causal = 0;
  constexpr int SWZ_K = (D == 128) ? 15 : 7;  // K image rows are 2*D bytes
  constexpr int SWZ_V = 7;                    // V^T image rows are 128 bytes
  constexpr int PT = (KVBLK * D / 8) / NT;
  constexpr int QROWS = NT / 2;  // q rows per workgroup (32 per wave)
  // The image-form kernels combine the lane halves of the row max and the
  // row sum with ba_half_pair (v_permlane32_swap) instead of __shfl_xor
  // (ds_bpermute_b32 + s_waitcnt lgkmcnt(0), which drains the V fragment
  // reads in flight): same bits, measured +0.9 % on top of the image
  // (profiles/fwd_vt/README.md).  The VSRC=0 kernels keep __shfl_xor, so
  // their code is the code the tuned numbers and the module path refer to.
  constexpr bool HSWAP = VSRC == 1;
  static_assert(PT >= 1, "tile must fill at least one chunk per thread");

  static_assert(KREG != 1 || (SUBT == 1 && NBUF == 2 && VPATH == 0),
                "KREG=1 path: SUBT=1, NBUF=2, V^T image only");
  static_assert(KREG != 2 || (SUBT == 1 && NBUF == 4 && VPATH == 0),
                "KREG=2 path: SUBT=1, NBUF=4 (cross-barrier prefetch)");
  static_assert(VSRC == 0 || (VPATH == 0 && SUBT == 1 && KREG == 0 &&
                              KVBLK == BA_VT_KVBLK),
                "the V^T image source: b128-read V^T LDS image, SUBT=1");
  // single LDS object: [NBUF buffers][K row-major | V transposed][KVBLK*D]
  // (KREG=1: V transposed only)
  constexpr int IMGS_F = (KREG == 1) ? 1 : 2;
  __shared__ T lds[NBUF * IMGS_F * KVBLK * D];
  auto ldsK = [&](int buf) -> T* { return lds + buf * (IMGS_F * KVBLK * D); };
  auto ldsVT = [&](int buf) -> T* {
    return lds + buf * (IMGS_F * KVBLK * D) + (KREG == 1 ? 0 : KVBLK * D);
  };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31;
  const int hi = lane >> 5;
  const int n = blockIdx.y;
  const int b = blockIdx.z;
  const int qb = blockIdx.x * QROWS + wave * 32;
  const int q_row = qb + l31;

  const T* qp = q + (int64_t)b * q_sb + (int64_t)n * q_sh;
  // grouped-query heads: q head n attends KV head n / G (wave-uniform,
  // once per workgroup); q, o, lse and the carry-in state stay on n
  const int nkv = n / G;
  const T* kp = k + (int64_t)b * k_sb + (int64_t)nkv * k_sh;
  const T* vp = v + (int64_t)b * v_sb + (int64_t)nkv * v_sh;

  // Q fragments: B-operand of S^T = mfma(K, Q); lane holds q row q_row,
  // elements d = 16*s + 8*hi + j  (8 contiguous -> one 16B load)
  frag qf[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    if (q_row < Sq) {
      const T* src = qp + (int64_t)q_row * q_ss + 16 * s + 8 * hi;
      qf[s] = __builtin_bit_cast(frag, *(const u32x4_t*)src);
    } else {
      u32x4_t z = {0, 0, 0, 0};
      qf[s] = __builtin_bit_cast(frag, z);
    }
  }

  const float c2 = scale * BA_LOG2E;  // exp2-domain scale
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

  const int kv_limit =
      causal ? min(Sk, (int)(blockIdx.x + 1) * QROWS) : Sk;
  const int nt_shape = (kv_limit + KVBLK - 1) / KVBLK;
  int2 trange = {0, nt_shape};
  // segment form: this lane's q id, the wave's (min, max) of them, the kv
  // ids and tile summaries of this batch row, and the block's tile range
  int qid = 0, wq_min = 0, wq_max = 0;
  const int32_t* kseg = nullptr;
  const int2* tmm = nullptr;
  bool seg_mask = false;  // the current tile needs the id compare
  if constexpr (HAS_SEG) {
    const ba_seg_args sg = ba_seg_of(seg...);
    const int2 r = sg.blk_range[(int64_t)b * gridDim.x + blockIdx.x];
    trange.x = r.x;
    trange.y = min(trange.y, r.y);
    if (trange.x >= trange.y) {
      // nothing visible to any row of this workgroup (uniform: no barrier
      // has been reached): o = 0, lse = -inf / a fresh empty state / the
      // carried state as it is
      if (q_row < Sq && !(OUT_STATE && carry_in)) {
        float* row = OUT_STATE
                         ? st_acc + b * a_sb + (int64_t)q_row * a_ss + n * a_sh
                         : o + (((int64_t)b * Sq + q_row) * N + n) * D;
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
          for (int r2 = 0; r2 < 16; ++r2) row[dt * 32 + ba_crow(r2, hi)] = 0.f;
        if (hi == 0) {
          if (OUT_STATE) {
            st_m[b * ml_sb + n * ml_sh + q_row] = BA_NEG_BIG;
            st_l[b * ml_sb + n * ml_sh + q_row] = 0.f;
          } else {
            lse[((int64_t)b * N + n) * Sq + q_row] = -__builtin_inff();
          }
        }
      }
      return;
    }
    qid = sg.q_seg[b * sg.q_sb + min(q_row, Sq - 1)];
    ba_wave_minmax(qid, wq_min, wq_max);
    kseg = sg.kv_seg + b * sg.kv_sb;
    tmm = sg.tile_mm + (int64_t)b * ((Sk + KVBLK - 1) / KVBLK);
  }
  // band form: the block's tile range is arithmetic (band_support.h)
  ba_band_args bd = {0, 0};
  bool band_full = false;  // the current tile holds no masked entry
  if constexpr (HAS_BAND) {
    bd = ba_band_of(seg...);
    const ba_tile_range r = ba_band_block_tiles(blockIdx.x, bd, Sq, Sk);
    trange.x = r.lo;
    trange.y = r.hi;
    if (trange.x >= trange.y) {
      // workgroup-uniform, no barrier yet; what the segment form writes
      if (q_row < Sq && !(OUT_STATE && carry_in)) {
        float* row = OUT_STATE
                         ? st_acc + b * a_sb + (int64_t)q_row * a_ss + n * a_sh
                         : o + (((int64_t)b * Sq + q_row) * N + n) * D;
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
          for (int r2 = 0; r2 < 16; ++r2) row[dt * 32 + ba_crow(r2, hi)] = 0.f;
        if (hi == 0) {
          if (OUT_STATE) {
            st_m[b * ml_sb + n * ml_sh + q_row] = BA_NEG_BIG;
            st_l[b * ml_sb + n * ml_sh + q_row] = 0.f;
          } else {
            lse[((int64_t)b * N + n) * Sq + q_row] = -__builtin_inff();
          }
        }
      }
      return;
    }
  }
  const int t_first = HAS_MASK ? trange.x : 0;
  const int nt = HAS_MASK ? trange.y : nt_shape;
  static_assert(SUBT != 2 || (NBUF == 4 && VPATH == 0),
                "the T15 pipeline needs NBUF=4 and the V^T image");
  static_assert(SUBT != 3 || (NBUF == 4 && VPATH == 0 && NT == 256),
                "SUBT=3: NT=256 (1 wave/SIMD), NBUF=4, V^T image");

  // ---- the steps, one definition each: every SUBT/KREG body below is a
  // sequence of these.  Always inlined, so a body compiles as if the steps
  // were written out in it; their shapes (what is a parameter, where a loop
  // sits) are the ones that leave the default variant's code as it was,
  // see profiles/fwd_kernel/README.md before reshaping one.
#define BA_STEP __attribute__((always_inline))
  // K fragment s (A operand of S^T) of the 32-kv subtile (buf, kvs)
  auto k_frag = [&](int buf, int kvs, int s) BA_STEP {
    return ba_ld_rowslice<T, D, SWZ_K>(ldsK(buf), kvs * 32 + l31,
                                       16 * s + 8 * hi);
  };
  auto load_kfrags = [&](int buf, int kvs, frag* kf) BA_STEP {
#pragma unroll
    for (int s = 0; s < D / 16; ++s) kf[s] = k_frag(buf, kvs, s);
  };
  // ... of the subtile after (t, kvs): (t,0) -> (t,1) -> (t+1,0)
  auto load_next_kfrags = [&](int t, int kvs, frag* kf) BA_STEP {
    const int nt_t = (kvs == 0) ? t : t + 1;
    if (nt_t < nt) load_kfrags(nt_t % NBUF, kvs ^ 1, kf);
  };
  // S^T = mfma(K, Q) of one subtile (raw, unscaled scores), K fragments
  // from registers / each read from LDS right before its MFMA
  auto qk_regs = [&](const frag* kf) BA_STEP {
    f32x16_t s = (f32x16_t)(0.f);
#pragma unroll
    for (int i = 0; i < D / 16; ++i) s = MT::mma(kf[i], qf[i], s);
    return s;
  };
  auto qk_lds = [&](int buf, int kvs) BA_STEP {
    f32x16_t s = (f32x16_t)(0.f);
#pragma unroll
    for (int i = 0; i < D / 16; ++i)
      s = MT::mma(k_frag(buf, kvs, i), qf[i], s);
    return s;
  };
  // boundary mask of the subtile at kv rows [base + off, +32)
  auto mask_sub = [&](f32x16_t& s, int base, int off) BA_STEP {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kv_g = base + off + ba_crow(r, 0) + 4 * hi;
      if (!(kv_g < Sk && (!causal || kv_g <= q_row))) s[r] = BA_NEG_BIG;
      if constexpr (HAS_SEG) {
        if (seg_mask && kseg[min(kv_g, Sk - 1)] != qid) s[r] = BA_NEG_BIG;
      }
      if constexpr (HAS_BAND) {
        if (!ba_band_visible(q_row, kv_g, bd)) s[r] = BA_NEG_BIG;
      }
    }
  };
  // row max in the exp2 domain.  The softmax scale is folded into the exp
  // argument (exp2+fma): the max is taken on RAW scores (max commutes with
  // c2 > 0), the scale costs one multiply on the max instead of 16 per
  // subtile
  auto row_max2 = [&](const f32x16_t& s) BA_STEP {
    float tm = ba_max16(s);
    if (HSWAP) {
      float lo, hi2;
      ba_half_pair(tm, lo, hi2);
      tm = fmaxf(lo, hi2);
    } else {
      tm = fmaxf(tm, __shfl_xor(tm, 32));
    }
    return tm * c2;
  };
  // online-softmax rescale (lane-local), defer-max (T13): skip the O/l
  // rescale while the running max grows by <= THR (exp2 domain); P is then
  // bounded by 2^THR instead of 1, which the fp32 accumulate absorbs.
  // Decision taken BEFORE these scores are exponentiated (the
  // textbook-safe order); wave-uniform.
  constexpr float DEFER_THR = 8.f;
  auto rescale = [&](float tm) BA_STEP {
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
  };
  // the rest of a subtile's softmax once its max is known: rescale, exp2
  // with the row sum, P -> fragments
  auto softmax_tail = [&](f32x16_t& s, float tm, frag* pf) BA_STEP {
    rescale(tm);
    float rowsum = 0.f;
    // band form, full tile (wave-uniform): no entry is masked and every
    // row's max is a real score after the rescale above, so the plain exp
    // serves and the select below stays out of the steady loop
    if (HAS_BAND && band_full) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = ba_exp2(__builtin_fmaf(s[r], c2, -m2));
        rowsum += s[r];
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        // segment form: a masked entry weighs exactly 0 even while the
        // row's running max is still at the masked level (a row whose tiles
        // so far held no visible key), where the exponent below would not
        // be small
        if constexpr (HAS_MASK) {
          const bool masked = s[r] == BA_NEG_BIG;
          s[r] = masked ? 0.f : ba_exp2(__builtin_fmaf(s[r], c2, -m2));
        } else {
          s[r] = ba_exp2(__builtin_fmaf(s[r], c2, -m2));
        }
        rowsum += s[r];
      }
    }
    if (HSWAP) {
      float lo, hi2;
      ba_half_pair(rowsum, lo, hi2);
      rowsum = lo + hi2;
    } else {
      rowsum += __shfl_xor(rowsum, 32);
    }
    lsum += rowsum;
    ba_build_frag_pair<T>(s, pf);
  };
  // V fragment (A operand of O^T) of buffer `buf`: this lane's d row
  // `drow` = 32 dt + l31, kv columns [kvc, +16)
  auto v_frag = [&](int buf, int drow, int kvc) BA_STEP -> frag {
    if (VPATH == 0)
      return ba_ld_rowslice<T, KVBLK, SWZ_V, 7>(ldsVT(buf), drow, kvc + 8 * hi);
    return ba_ld_tr16_frag<T, D>(ldsVT(buf), lane, kvc, drow & ~31);
  };
  // O^T += mfma(V^T, P^T) of one subtile on prefetched V fragments.  (The
  // LDS form is the same two loops around v_frag, written in its callers: a
  // helper holding the loops, called last in the SUBT=1 subtile loop, moves
  // that loop's blocks and with them the D=64 default kernels' code.)
  auto pv_regs = [&](const frag* vv, const frag* pf) BA_STEP {
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
      for (int u = 0; u < 2; ++u)
        ot[dt] = MT::mma(vv[dt * 2 + u], pf[u], ot[dt]);
  };
  // (row, 8-element column) of this thread's chunk c of a staged tile
  struct chunk_rc {
    int row, col8;
  };
  auto stage_rc = [&](int c) BA_STEP {
    const int flat = tid + c * NT;
    return chunk_rc{flat / (D / 8), flat % (D / 8)};
  };
#undef BA_STEP

  // ---- SUBT=2/3 pipeline stage 1: the previous subtile's raw scores and
  // its metadata, finished during the next subtile's QK cluster
  f32x16_t stP;
  int p_kv0 = -1;   // -1 = pipeline empty
  int p_cur = 0;
  bool p_full = false;
  auto push_scores = [&](const f32x16_t& s, int kv0s, int buf, bool full) {
    stP = s;
    p_kv0 = kv0s;
    p_cur = buf;
    p_full = full;
  };
  auto finish_subtile = [&]() {
    if (!p_full) mask_sub(stP, p_kv0, 0);
    frag pf[2];
    softmax_tail(stP, row_max2(stP), pf);
    const int kvs_l = (p_kv0 / 32) & 1;  // subtile index within its tile
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt) {
      const int drow = dt * 32 + l31;
#pragma unroll
      for (int u = 0; u < 2; ++u)
        ot[dt] = MT::mma(v_frag(p_cur, drow, kvs_l * 32 + 16 * u), pf[u],
                         ot[dt]);
    }
  };

  // ---- SUBT=3 additional state: stage 2 (P fragments of subtile k-2
  // awaiting PV) and the register-prefetched K/V operands
  frag pvf[2];                     // P fragments awaiting PV
  frag kfP[SUBT == 3 ? D / 16 : 1];  // prefetched K frags (QK of phase k)
  frag vvP[SUBT == 3 ? D / 16 : 1];  // prefetched V rowslices (PV operands)
  int v_kv0 = -1;                  // -1 = stage 2 empty

  // one SUBT=3 pipeline phase for subtile (t, kvs) using buffer `cur3`:
  // QK(k) on prefetched kfP -> kf prefetch for k+1 -> softmax part 1 of
  // stP (mask+max) -> PV(k-2) on prefetched vvP -> softmax part 2
  // (rescale ordered AFTER the PV, exp2, rowsum, pack -> pvf) -> vv
  // prefetch for the new pf -> rotate stage 1.
  // `steady` folds the pipeline-occupancy guards away at the two
  // steady-state call sites (t >= 1: both stages provably occupied) —
  // round-3 prerequisite: the steady loop must be straight-line for the
  // hand-scheduled .s body
  auto phase3 = [&](bool steady, int t, int kvs, int cur3, bool full) {
    // --- QK(k) on the prefetched K fragments, then re-fill them for
    // the next subtile (WAR on kfP; a full phase of flight).
    // NOTE (measured): pinning this cadence with per-op
    // volatile asm does NOT help — the accumulators cross the C/asm
    // boundary through 100-470 register copies per phase and the C
    // softmax is not gap-packed.  The plain form below is the honest
    // compiler-scheduled 3-stage pipeline; the hand-placed version is
    // the round-3 full-asm body.
    const f32x16_t stQ = qk_regs(kfP);
    load_next_kfrags(t, kvs, kfP);
    // --- softmax part 1 on stP: mask + row max (no ot/m2 writes)
    float tm = BA_NEG_BIG;
    if (steady || p_kv0 >= 0) {
      if (!p_full) mask_sub(stP, p_kv0, 0);
      tm = row_max2(stP);
    }
    // --- PV(k-2) on the prefetched operands
    if (steady || v_kv0 >= 0) pv_regs(vvP, pvf);
    // --- softmax part 2: rescale (safe now: the PV above has landed),
    // exp2, rowsum, pack; then prefetch the new pf's V operands
    if (steady || p_kv0 >= 0) {
      softmax_tail(stP, tm, pvf);
      v_kv0 = p_kv0;
      const int kvs_l = (p_kv0 / 32) & 1;
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int u = 0; u < 2; ++u)
          vvP[dt * 2 + u] = v_frag(p_cur, dt * 32 + l31, kvs_l * 32 + 16 * u);
    }
    // --- rotate stage 1
    push_scores(stQ, t * KVBLK + kvs * 32, cur3, full);
  };

  // staging lane offsets are loop-invariant; computing them once turns an
  // in-range tile's addresses into (scalar tile base) + (u32 lane offset),
  // which the compiler emits as saddr-form global_loads — the per-tile
  // 64-bit address recompute (~32 VALU ops) leaves the steady loop, and
  // the issue port is the oversubscribed resource there (ACTIVE+STALL
  // ~124% of SIMD issue slots at 2 waves, profiles/r02/sq_wait_taxonomy)
  uint32_t k_loff[PT], v_loff[PT];
#pragma unroll
  for (int c = 0; c < PT; ++c) {
    const auto [row, col8] = stage_rc(c);
    k_loff[c] = (uint32_t)((row * k_ss + col8 * 8) * (int64_t)sizeof(T));
    v_loff[c] = (uint32_t)((row * v_ss + col8 * 8) * (int64_t)sizeof(T));
  }
  const bool stage_lin =
      (int64_t)(KVBLK - 1) * k_ss * (int64_t)sizeof(T) + 16 <= 0xffffffffLL &&
      (VSRC == 1 ||
       (int64_t)(KVBLK - 1) * v_ss * (int64_t)sizeof(T) + 16 <= 0xffffffffLL);
  auto issue_loads = [&](int tile, u32x4_t* kreg, u32x4_t* vreg) {
    const int kv0 = tile * KVBLK;
    // image source: chunk c of the tile's block, a scalar block base plus
    // the lane's invariant offset.  The last block is zero-padded to 64
    // columns, so no tile needs a clamp.
    if (VSRC == 1) {
      const char* vb = (const char*)(vp + tile * ba_vt_block_elems(D));
#pragma unroll
      for (int c = 0; c < PT; ++c)
        vreg[c] = *(const u32x4_t*)(vb + (uint32_t)((tid + c * NT) * 16));
    }
    // the fast path's invariant offsets cost live registers the SUBT=2/3
    // pipelined variants cannot spare (they spill); production SUBT=1 only
    if (SUBT == 1 && stage_lin && kv0 + KVBLK <= Sk) {
      const char* kb = (const char*)(kp + (int64_t)kv0 * k_ss);
      const char* vb = (const char*)(vp + (int64_t)kv0 * v_ss);
#pragma unroll
      for (int c = 0; c < PT; ++c) {
        if (KREG != 1) kreg[c] = *(const u32x4_t*)(kb + k_loff[c]);
        if (VSRC == 0) vreg[c] = *(const u32x4_t*)(vb + v_loff[c]);
      }
      return;
    }
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      const auto [row, col8] = stage_rc(c);
      // clamped index instead of a guarded load: the guard compiles to
      // an exec-mask branch around every load pair (serialising the
      // staging); clamped rows re-load row Sk-1, whose values are
      // nullified by the kv-range mask (p = 0) in the softmax
      const int kvg = kv0 + row;
      const int kvc = kvg < Sk ? kvg : (Sk - 1);
      if (KREG != 1)
        kreg[c] = *(const u32x4_t*)(kp + (int64_t)kvc * k_ss + col8 * 8);
      if (VSRC == 0)
        vreg[c] = *(const u32x4_t*)(vp + (int64_t)kvc * v_ss + col8 * 8);
    }
  };
  auto write_lds = [&](int buf, const u32x4_t* kreg, const u32x4_t* vreg) {
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      const auto [row, col8] = stage_rc(c);
      if (KREG != 1) {
        const int byte = ba_swz<SWZ_K>(row * (2 * D) + col8 * 16, row);
        *(u32x4_t*)((char*)ldsK(buf) + byte) = kreg[c];
      }
      if (VSRC == 1) {
        // the address ba_st_transposed gives these eight elements: the
        // swizzle moves whole 16-byte granules, so the chunk stays whole
        const int flat = tid + c * NT;
        const int byte = ba_swz<SWZ_V, 7>(flat * 16, flat / (KVBLK / 8));
        *(u32x4_t*)((char*)ldsVT(buf) + byte) = vreg[c];
      } else if (VPATH == 0)
        ba_st_transposed<T, KVBLK, SWZ_V, 7>(ldsVT(buf), row, col8 * 8, vreg[c]);
      else
        ba_st_tr16row<T, D>(ldsVT(buf), row, col8 * 8, vreg[c]);
    }
  };
  // KREG: one K subtile straight into the A-fragment registers (lane
  // reads its own kv row; clamped like the staging)
  auto load_k_sub = [&](int tile, int kvs, frag* dst) {
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      const int kvg = tile * KVBLK + kvs * 32 + l31;
      const int kvc = kvg < Sk ? kvg : (Sk - 1);
      dst[s] = __builtin_bit_cast(
          frag, *(const u32x4_t*)(kp + (int64_t)kvc * k_ss + 16 * s + 8 * hi));
    }
  };

  frag kfr[KREG == 1 ? 2 : 1][D / 16];  // KREG: resident K fragments
  {  // prologue: tiles 0..NBUF-2
    u32x4_t kreg[PT], vreg[PT];
    issue_loads(t_first, kreg, vreg);
    write_lds(0, kreg, vreg);
    if (KREG == 1) {
      load_k_sub(0, 0, kfr[0]);
      load_k_sub(0, 1, kfr[KREG == 1 ? 1 : 0]);
    }
    if (NBUF == 4 && nt > 1) {
      issue_loads(1, kreg, vreg);
      write_lds(1, kreg, vreg);
    }
    __syncthreads();
    // prime the prefetched K operands with (tile 0, subtile 0)
    if (KREG == 2) load_kfrags(0, 0, kfr[0]);
    if (SUBT == 3) load_kfrags(0, 0, kfP);
  }
  // static priority for the younger dispatch half (T5 static form):
  // wave-uniform condition via readfirstlane, one s_setprio, no flips
  if (NT == 512 && __builtin_amdgcn_readfirstlane(threadIdx.x) >= 256)
    __builtin_amdgcn_s_setprio(1);

  constexpr int AHEAD = NBUF == 4 ? 2 : 1;
  // the tile loop is hand-unrolled by the buffer period so `cur` (and the
  // staging write buffer) are compile-time per copy: the LDS buffer offset
  // folds into the ds_read/ds_write offset immediates instead of costing a
  // v_or per access — ~40 issue slots per tile in an issue-bound loop
  auto tile_body = [&](int t, auto curc) {
    const int cur = ba_buf_of(curc);  // compile-time literal for ba_ic
    const int kv0 = t * KVBLK;
    const bool has_next = (t + AHEAD) < nt;
    u32x4_t kreg[PT], vreg[PT];
    if (has_next) issue_loads(t + AHEAD, kreg, vreg);

    bool active, full;
    if constexpr (HAS_SEG) {
      // segment form: the tile's (min, max) ids against the wave's; a full
      // tile also has one id on both sides
      const int2 mm = tmm[t];
      seg_mask = !(mm.x == mm.y && wq_min == wq_max && mm.x == wq_min);
      active = (!causal || (kv0 <= qb + 31)) && mm.y >= wq_min &&
               mm.x <= wq_max;
      full = (kv0 + KVBLK <= Sk) && (!causal || (kv0 + KVBLK - 1 <= qb)) &&
             !seg_mask;
    } else if constexpr (HAS_BAND) {
      // band form: the tile against the band of the wave's 32 rows
      active = ba_band_wave_active(qb, kv0, bd);
      full = (kv0 + KVBLK <= Sk) && ba_band_wave_inside(qb, kv0, bd);
      band_full = full;
    } else {
      active = !causal || (kv0 <= qb + 31);
    }
    if (active) {
      // a full tile needs no mask: inside Sk and, if causal, at or below
      // the diagonal for every q row of this wave.  (SUBT=0 takes its own
      // copy after its QK MFMAs: reading this one costs its register-tight
      // tr16 kernels 4 to 8 bytes more scratch.)
      if constexpr (!HAS_MASK)
        full = (kv0 + KVBLK <= Sk) && (!causal || (kv0 + KVBLK - 1 <= qb));
      if (SUBT == 3) {
        // NOTE: a C-level warmup peel (separate guarded/steady calls)
        // measured -48% — four inlined phase copies bloat the loop body.
        // The peel belongs at the .s level (round 3), where the warmup
        // runs before the loop label.
        [[clang::always_inline]] phase3(false, t, 0, cur, full);
        [[clang::always_inline]] phase3(false, t, 1, cur, full);
      } else if (SUBT == 2) {
        // ---- T15 pipeline: QK(j) fills while FINISH+PV(j-1) retire
#pragma unroll
        for (int kvs = 0; kvs < 2; ++kvs) {
          const f32x16_t stQ = qk_lds(cur, kvs);
          if (p_kv0 >= 0) [[clang::always_inline]] finish_subtile();
          push_scores(stQ, kv0 + kvs * 32, cur, full);
        }
      } else if (SUBT == 1) {
        // ---- per-subtile pipeline: {QK, softmax, PV} x 2, independent
        // chains so the scheduler overlaps PV(0) with QK(1)
#pragma unroll
        for (int kvs = 0; kvs < 2; ++kvs) {
          frag* kres = kfr[KREG == 1 ? kvs : 0];
          f32x16_t st = KREG ? qk_regs(kres) : qk_lds(cur, kvs);
          // KREG=1: this subtile's K block is consumed — re-issue its
          // global loads for the next tile at once (WAR on the same
          // registers; HBM latency hides under softmax + PV + staging)
          if (KREG == 1 && has_next) load_k_sub(t + AHEAD, kvs, kres);
          // KREG=2: re-fill the fragment set from LDS one subtile ahead
          // (tile t+1's buffer was staged two tiles ago, ordered by the
          // per-tile barrier)
          if (KREG == 2) load_next_kfrags(t, kvs, kres);
          if (!full) mask_sub(st, kv0, kvs * 32);
          frag pf[2];
          softmax_tail(st, row_max2(st), pf);
#pragma unroll
          for (int dt = 0; dt < D / 32; ++dt) {
            const int drow = dt * 32 + l31;
#pragma unroll
            for (int u = 0; u < 2; ++u)
              ot[dt] = MT::mma(v_frag(cur, drow, kvs * 32 + 16 * u), pf[u],
                               ot[dt]);
          }
        }
      } else {
        // ---- SUBT=0: joint softmax over both subtiles, on scores
        // pre-scaled into the exp2 domain (+ mask only on boundary tiles);
        // the two QK chains interleave per K fragment
        f32x16_t st[2] = {(f32x16_t)(0.f), (f32x16_t)(0.f)};
#pragma unroll
        for (int s = 0; s < D / 16; ++s) {
          frag k0 = ba_ld_rowslice<T, D, SWZ_K>(ldsK(cur), l31, 16 * s + 8 * hi);
          frag k1 =
              ba_ld_rowslice<T, D, SWZ_K>(ldsK(cur), 32 + l31, 16 * s + 8 * hi);
          st[0] = MT::mma(k0, qf[s], st[0]);
          st[1] = MT::mma(k1, qf[s], st[1]);
        }
        const bool full0 =
            (kv0 + KVBLK <= Sk) && (!causal || (kv0 + KVBLK - 1 <= qb));
        if (full0) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            st[0][r] *= c2;
            st[1][r] *= c2;
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kv_g0 = kv0 + ba_crow(r, 0) + 4 * hi;
            const int kv_g1 = kv_g0 + 32;
            st[0][r] = (kv_g0 < Sk && (!causal || kv_g0 <= q_row))
                           ? st[0][r] * c2
                           : BA_NEG_BIG;
            st[1][r] = (kv_g1 < Sk && (!causal || kv_g1 <= q_row))
                           ? st[1][r] * c2
                           : BA_NEG_BIG;
          }
        }
        float tm = BA_NEG_BIG;
#pragma unroll
        for (int r = 0; r < 16; ++r) tm = fmaxf(tm, fmaxf(st[0][r], st[1][r]));
        tm = fmaxf(tm, __shfl_xor(tm, 32));
        rescale(tm);
        float rowsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          st[0][r] = ba_exp2(st[0][r] - m2);
          st[1][r] = ba_exp2(st[1][r] - m2);
          rowsum += st[0][r] + st[1][r];
        }
        rowsum += __shfl_xor(rowsum, 32);
        lsum += rowsum;

        // ---- P -> fragments, O^T += mfma(V^T, P^T); the two subtiles
        // alternate per u (the accumulation order of this form)
        frag pf[2][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) ba_build_frag_pair<T>(st[j], pf[j]);
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt) {
          const int drow = dt * 32 + l31;
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const frag v0 = v_frag(cur, drow, 16 * u);
            const frag v1 = v_frag(cur, drow, 32 + 16 * u);
            ot[dt] = MT::mma(v0, pf[0][u], ot[dt]);
            ot[dt] = MT::mma(v1, pf[1][u], ot[dt]);
          }
        }
      }
    }

    if (has_next) write_lds((cur + AHEAD) % NBUF, kreg, vreg);
    // SUBT=2 reads the previous tile's V one subtile late: barrier every
    // tile so the rewrite (2 buffers ahead) never crosses those reads
    if (SUBT == 2 || SUBT == 3 || KREG == 2 || NBUF == 2 || (t & 1) ||
        t + 1 >= nt)
      __syncthreads();
  };
  if constexpr (SUBT == 1) {
    // Fix the steady loop's code placement.  The loop takes ~15 branches
    // per tile and its rate depends on where their targets fall in the
    // fetch lines: moving the identical loop by 12 bytes (27 prologue
    // instructions for the n / G above) measured -3% on the headline
    // forward, and padding it back restored the rate (DESIGN §11,
    // profiles/gqa/).  The directive lands in the loop's preheader, so
    // the loop's offset within a 128-byte line no longer follows the
    // prologue's length.  Nothing in the language ties the statement to
    // the loop header: the compiler is free to put preheader
    // instructions after it, so this holds for the code a given
    // compiler emits, and was checked in the disassembly of the default
    // variant <0,1,512,2,0> (D=64/128, fp16/bf16, both OUT_STATE forms).
    // For its D=128 carry-in form (the ring path) the result is the
    // placement the tuned numbers were measured at.  The pad is a few
    // s_nops executed once per workgroup.
    // The header itself is not 128-byte aligned in any of these kernels
    // (D=128 carry-in: 84 mod 128 with VSRC=0, 60 with VSRC=1).  For the
    // VSRC=1 kernel, padding the preheader so that the header lands at 88
    // or exactly 0 measured the same rate as 60, and 4 measured -2 %
    // (profiles/fwd_vt/README.md): what matters is that the placement is
    // a measured one and stays put, which this directive provides.
    asm volatile(".p2align 7");
    // (segment form: the range may start at any tile; the buffer of a copy
    // is its position in the unrolled body, not the tile's parity)
    for (int tb = t_first; tb < nt; tb += NBUF) {
      [[clang::always_inline]] tile_body(tb, ba_ic<0>{});
      if (tb + 1 < nt) [[clang::always_inline]] tile_body(tb + 1, ba_ic<1 % NBUF>{});
      if (NBUF > 2) {
        if (tb + 2 < nt) [[clang::always_inline]] tile_body(tb + 2, ba_ic<2 % NBUF>{});
        if (tb + 3 < nt) [[clang::always_inline]] tile_body(tb + 3, ba_ic<3 % NBUF>{});
      }
    }
  } else {
    // the pipelined variants (SUBT=2/3) carry register state across tile
    // boundaries; unrolled copies quadruple it into scratch spills, so
    // they keep the rolled loop with a runtime buffer index
    for (int t = 0; t < nt; ++t)
      [[clang::always_inline]] tile_body(t, ba_dyn{t % NBUF});
  }
  if (SUBT == 2 && p_kv0 >= 0) finish_subtile();  // drain the pipeline
  if (SUBT == 3) {  // drain both pending stages (PV first: scale order)
    if (v_kv0 >= 0) pv_regs(vvP, pvf);
    if (p_kv0 >= 0) finish_subtile();
  }

  // ---- epilogue
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
      // segment form: a row that saw no key has l = 0: o = 0, lse = -inf
      float inv_l = 1.f / lsum;
      if constexpr (HAS_MASK) inv_l = lsum == 0.f ? 0.f : inv_l;
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

// finalize: o = acc / l (cast to T), lse = ln2 * (m + log2(l)).
// acc/m/l are the FULL chunk (contiguous); one wave row-group per row.
template <typename T, int D>
__global__ void attn_fwd_finalize_kernel(
    const float* __restrict__ acc, const float* __restrict__ m,
    const float* __restrict__ l, T* __restrict__ o, float* __restrict__ lse,
    int S, int N) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  constexpr int LPR = D / 16;           // lanes per row (8 for D=128)
  const int rows_per_wave = 64 / LPR;   // 8
  const int row_in = wave * rows_per_wave + lane / LPR;
  const int sub = lane % LPR;
  const int s = blockIdx.x * 4 * rows_per_wave + row_in;
  const int n = blockIdx.y, b = blockIdx.z;
  if (s >= S) return;
  const float lv = l[((int64_t)b * N + n) * S + s];
  // l == 0: a row that saw no key in any round (possible with segment ids
  // in direct tile calls only): o = 0, and lse below comes out -inf
  const float inv_l = lv > 0.f ? 1.f / lv : 0.f;
  const float* arow = acc + (((int64_t)b * S + s) * N + n) * D + sub * 16;
  T* orow = o + (((int64_t)b * S + s) * N + n) * D + sub * 16;
#pragma unroll
  for (int j = 0; j < 16; ++j) orow[j] = (T)(arow[j] * inv_l);
  if (sub == 0)
    lse[((int64_t)b * N + n) * S + s] =
        BA_LN2 * (m[((int64_t)b * N + n) * S + s] + log2f(lv));
}

// the empty carry-in state: acc = 0, l = 0, m = the level a carry_in = 0
// call starts from.  One thread per V floats of acc (V = 4 where the state
// is 16-byte aligned, else 1); the threads of d = 0 also write m and l.
template <int V>
__global__ __launch_bounds__(256) void attn_fwd_state_init_kernel(
    float* __restrict__ acc, float* __restrict__ m, float* __restrict__ l,
    int S, int N, int D, int64_t a_sb, int64_t a_ss, int64_t a_sh,
    int64_t ml_sb, int64_t ml_sh) {
  const int dv = D / V;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= (int64_t)S * N * dv) return;
  const int d = (int)(i % dv) * V;
  const int n = (int)((i / dv) % N);
  const int s = (int)(i / ((int64_t)dv * N));
  float* row = acc + b * a_sb + (int64_t)s * a_ss + n * a_sh + d;
  if (V == 4) {
    *(float4*)row = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    row[0] = 0.f;
  }
  if (d == 0) {
    m[b * ml_sb + n * ml_sh + s] = BA_NEG_BIG;
    l[b * ml_sb + n * ml_sh + s] = 0.f;
  }
}

// V^T image pre-pass (layout: vt_image.h).  One workgroup per (kv tile, kv
// head, batch): the 64 x D tile goes through LDS with the transposed
// staging write and the row-slice read the forward kernel uses for the same
// image, so both global sides are 16 B per lane and coalesced.  Rows at
// kv >= Sk are not read; their columns are written as zeros.  `img_elems`
// is the capacity of `img` in elements: a chunk that would end past it is
// not written.  Memory-bound, one pass over V in and one out.
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_vt_image_kernel(
    const T* __restrict__ v, T* __restrict__ img, int Sk, int Nk,
    int64_t v_sb, int64_t v_ss, int64_t v_sh, int64_t img_elems) {
  constexpr int KVBLK = BA_VT_KVBLK;
  constexpr int NT = 256;
  constexpr int PT = (KVBLK * D / 8) / NT;
  __shared__ T lds[KVBLK * D];
  const int tid = threadIdx.x;
  const int t = blockIdx.x, nkv = blockIdx.y, b = blockIdx.z;
  const T* vp = v + (int64_t)b * v_sb + (int64_t)nkv * v_sh;
#pragma unroll
  for (int c = 0; c < PT; ++c) {
    const int flat = tid + c * NT;
    const int row = flat / (D / 8), col8 = flat % (D / 8);
    const int kvg = t * KVBLK + row;
    u32x4_t chunk = {0, 0, 0, 0};
    if (kvg < Sk)
      chunk = *(const u32x4_t*)(vp + (int64_t)kvg * v_ss + col8 * 8);
    ba_st_transposed<T, KVBLK, 7, 7>(lds, row, col8 * 8, chunk);
  }
  __syncthreads();
  const int64_t blk = ba_vt_offset(Nk, Sk, D, b, nkv, (int64_t)t * KVBLK, 0);
#pragma unroll
  for (int c = 0; c < PT; ++c) {
    const int flat = tid + c * NT;  // chunk (d = flat / 8, kv8 = flat % 8)
    const auto f = ba_ld_rowslice<T, KVBLK, 7, 7>(lds, flat / (KVBLK / 8),
                                                  (flat % (KVBLK / 8)) * 8);
    const int64_t e = blk + (int64_t)flat * 8;
    if (e + 8 <= img_elems) *(u32x4_t*)(img + e) = __builtin_bit_cast(u32x4_t, f);
  }
}

// ---- segment-id pre-pass (layout: seg_support.h) ------------------------
// Step 1, one wave per 64-row tile of the streamed side: the tile's
// (min, max) id, and a per-batch-row flag raised where an id is smaller
// than its predecessor.  Rows past S repeat the last id.
__global__ __launch_bounds__(256) void seg_tile_minmax_kernel(
    const int32_t* __restrict__ ids, int64_t sb, int S, int ntiles,
    int2* __restrict__ mm, int* __restrict__ nonmono) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (t >= ntiles) return;
  const int i = min(t * BA_SEG_TILE + lane, S - 1);
  const int32_t* row = ids + b * sb;
  const int id = row[i];
  if (__any(row[max(i - 1, 0)] > id) && lane == 0) atomicOr(nonmono + b, 1);
  int mn, mx;
  ba_wave_minmax(id, mn, mx);
  if (lane == 0) mm[(int64_t)b * ntiles + t] = make_int2(mn, mx);
}

// Step 2, one workgroup per 256-row block of the owning side: the range
// [lo, hi) of streamed tiles whose (min, max) overlaps the block's.  Where
// the streamed ids are non-decreasing (packed documents, in every layout
// of the ring) the tile summaries are sorted and one thread finds the range
// by two binary searches; for one non-decreasing id sequence on both sides
// (a packed sequence attending itself) these are exactly the tiles that
// share an id with the block.  Otherwise the workgroup scans the summaries and the range is the hull of
// the overlapping tiles: conservative, still correct under the element
// mask.
__global__ __launch_bounds__(256) void seg_block_range_kernel(
    const int32_t* __restrict__ ids, int64_t sb, int S,
    const int2* __restrict__ mm, int ntiles, const int* __restrict__ nonmono,
    int2* __restrict__ range) {
  __shared__ int s_min, s_max, s_lo, s_hi;
  const int tid = threadIdx.x, b = blockIdx.y;
  if (tid == 0) {
    s_min = INT32_MAX;
    s_max = INT32_MIN;
    s_lo = ntiles;
    s_hi = 0;
  }
  __syncthreads();
  int mn, mx;
  ba_wave_minmax(ids[b * sb + min((int)blockIdx.x * BA_SEG_BLOCK + tid, S - 1)],
                 mn, mx);
  if ((tid & 63) == 0) {
    atomicMin(&s_min, mn);
    atomicMax(&s_max, mx);
  }
  __syncthreads();
  const int bmin = s_min, bmax = s_max;
  const int2* m = mm + (int64_t)b * ntiles;
  int2* out = range + (int64_t)b * gridDim.x + blockIdx.x;
  if (!nonmono[b]) {
    if (tid == 0) {
      int lo = 0, hi = ntiles;  // first tile with max >= bmin
      while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (m[mid].y >= bmin) hi = mid; else lo = mid + 1;
      }
      int lo2 = lo, hi2 = ntiles;  // first tile with min > bmax
      while (lo2 < hi2) {
        const int mid = (lo2 + hi2) / 2;
        if (m[mid].x > bmax) hi2 = mid; else lo2 = mid + 1;
      }
      *out = make_int2(lo, lo2);
    }
    return;
  }
  for (int t = tid; t < ntiles; t += 256)
    if (m[t].y >= bmin && m[t].x <= bmax) {
      atomicMin(&s_lo, t);
      atomicMax(&s_hi, t + 1);
    }
  __syncthreads();
  if (tid == 0) *out = make_int2(s_lo, s_hi);
}

}  // namespace

// ranges of one side pair: `own` is the side whose 256-row blocks the
// kernel's workgroups hold, `str` the side they stream in 64-row tiles
int ba_seg_prepass(const int32_t* own, int64_t own_sb, int64_t S_own,
                   const int32_t* str, int64_t str_sb, int64_t S_str,
                   int64_t B, int32_t* flags, int32_t* tile_mm,
                   int32_t* blk_range, hipStream_t stream) {
  const int nt = (int)ba_seg_tiles(S_str), nb = (int)ba_seg_blocks(S_own);
  hipError_t e = hipMemsetAsync(flags, 0, (size_t)B * sizeof(int32_t), stream);
  if (e != hipSuccess)
    return ba_fail((int)e, "segment pre-pass memset failed: %s",
                   hipGetErrorString(e));
  seg_tile_minmax_kernel<<<dim3((unsigned)((nt + 3) / 4), (unsigned)B), 256, 0,
                           stream>>>(str, str_sb, (int)S_str, nt,
                                     (int2*)tile_mm, flags);
  seg_block_range_kernel<<<dim3((unsigned)nb, (unsigned)B), 256, 0, stream>>>(
      own, own_sb, (int)S_own, (const int2*)tile_mm, nt, flags,
      (int2*)blk_range);
  return ba_launch_status();
}

extern "C" const char* bahip_last_error(void) { return ba_g_err; }

// ---- forward launch layer ---------------------------------------------
// One field per attn_fwd_kernel parameter, in kernel order.  launch_fwd
// expands it into the <<<>>> call; the module-launched path hands it to
// the runtime as the packed kernarg buffer (explicit arguments only: the
// HIP runtime appends the hidden ones itself — verified by tools/asm_probe).
struct fwd_args {
  const void *q, *k, *v;
  float *o, *lse;
  int Sq, Sk, N, G;
  int64_t q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, v_sb, v_ss, v_sh;
  float scale;
  int causal;
  float *st_acc, *st_m, *st_l;
  int64_t a_sb, a_ss, a_sh, ml_sb, ml_sh;
  int carry_in;
};

using production_kernel_t = decltype(&attn_fwd_kernel<
    _Float16, 128, 64, 1, BA_FWD_PRODUCTION.vpath, BA_FWD_PRODUCTION.subt,
    BA_FWD_PRODUCTION.nt, BA_FWD_PRODUCTION.nbuf, BA_FWD_PRODUCTION.kreg>);
static_assert(offsetof(fwd_args, carry_in) + sizeof(int) ==
                      kernarg_size<production_kernel_t>::value &&
                  sizeof(fwd_args) ==
                      (kernarg_size<production_kernel_t>::value + 7) / 8 * 8,
              "fwd_args must mirror attn_fwd_kernel's parameter list");

// wave w of a workgroup owns 32 q rows: NT threads cover NT/2 rows
static dim3 fwd_grid(const fwd_args& a, int64_t B, int nt) {
  return dim3((unsigned)((a.Sq + nt / 2 - 1) / (nt / 2)), (unsigned)a.N,
              (unsigned)B);
}

template <typename T, int D, int OUT_STATE, int VPATH, int SUBT, int NT,
          int NBUF, int KREG, int VSRC = 0>
static void launch_fwd(const fwd_args& a, int64_t B, hipStream_t stream) {
  attn_fwd_kernel<T, D, 64, OUT_STATE, VPATH, SUBT, NT, NBUF, KREG, VSRC>
      <<<fwd_grid(a, B, NT), dim3(NT), 0, stream>>>(
          (const T*)a.q, (const T*)a.k, (const T*)a.v, a.o, a.lse, a.Sq, a.Sk,
          a.N, a.G, a.q_sb, a.q_ss, a.q_sh, a.k_sb, a.k_ss, a.k_sh, a.v_sb, a.v_ss,
          a.v_sh, a.scale, a.causal, a.st_acc, a.st_m, a.st_l, a.a_sb, a.a_ss,
          a.a_sh, a.ml_sb, a.ml_sh, a.carry_in);
}

// ---- segment-id form ----------------------------------------------------
// What a *_seg entry point adds to the plain call.
struct fwd_seg_call {
  const int32_t *q_seg, *kv_seg;
  int64_t q_sb, kv_sb;
  void* ws;
  int64_t ws_bytes;
};

// One of the two id pointers without the other is an error; both null is
// the plain call (0), both given the segment form (1).
static int seg_ids_given(const void* q_seg, const void* kv_seg, int* given) {
  if ((q_seg == nullptr) != (kv_seg == nullptr))
    return ba_fail(BAHIP_ERR_SEGMENT_IDS,
                   "segment ids: q_seg and kv_seg must both be given or both "
                   "be null (%s is null)",
                   q_seg ? "kv_seg" : "q_seg");
  *given = q_seg != nullptr;
  return 0;
}

// The forward with ids: the default variant only, V transposed in the
// kernel whatever BA_FWD_VT says (one kernel, so the results cannot depend
// on that knob), never the module kernel.  Pre-pass, then the forward, on
// the same stream.
// Both masked forms (segment ids, band) exist for the default variant only:
// 0 when the BA_FWD_* knobs select it, else the error naming the knob.
static int fwd_default_variant_only(const char* what) {
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
                   "%s=%d does not support %s (default forward variant only)",
                   sv.knob, sv.value, what);
  return 0;
}

static int fwd_seg_entry(const fwd_args& a, const fwd_seg_call& sc,
                         int out_state, int64_t B, int64_t Sq, int64_t Sk,
                         int64_t D, int dtype, hipStream_t stream) {
  if (int rc = fwd_default_variant_only("segment ids")) return rc;
  if (B < 1 || B > 65535 || Sq < 1 || Sk < 1)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "segment ids: unsupported shape B=%d Sq=%d Sk=%d", (int)B,
                   (int)Sq, (int)Sk);
  if (!sc.ws || sc.ws_bytes < ba_seg_ws_bytes(B, Sq, Sk))
    return ba_fail(BAHIP_ERR_WORKSPACE,
                   "segment workspace of %lld bytes is smaller than the %lld "
                   "needed",
                   (long long)(sc.ws ? sc.ws_bytes : 0),
                   (long long)ba_seg_ws_bytes(B, Sq, Sk));
  const ba_seg_ws_layout w = ba_seg_ws(B, Sq, Sk);
  int32_t* ws = (int32_t*)sc.ws;
  if (int rc = ba_seg_prepass(sc.q_seg, sc.q_sb, Sq, sc.kv_seg, sc.kv_sb, Sk,
                              B, ws + w.flags_kv, ws + w.kv_tile_mm,
                              ws + w.q_blk_range, stream))
    return rc;
  const ba_seg_args sg = {sc.q_seg, sc.kv_seg, sc.q_sb, sc.kv_sb,
                          (const int2*)(ws + w.kv_tile_mm),
                          (const int2*)(ws + w.q_blk_range)};
  return ba_dispatch_td(D, dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    constexpr int TD = decltype(td)::D;
    constexpr ba_fwd_variant P = BA_FWD_PRODUCTION;
    const dim3 grid = fwd_grid(a, B, P.nt);
    auto go = [&](auto kernel) {
      kernel<<<grid, dim3(P.nt), 0, stream>>>(
          (const T*)a.q, (const T*)a.k, (const T*)a.v, a.o, a.lse, a.Sq, a.Sk,
          a.N, a.G, a.q_sb, a.q_ss, a.q_sh, a.k_sb, a.k_ss, a.k_sh, a.v_sb,
          a.v_ss, a.v_sh, a.scale, a.causal, a.st_acc, a.st_m, a.st_l, a.a_sb,
          a.a_ss, a.a_sh, a.ml_sb, a.ml_sh, a.carry_in, sg);
    };
    if (out_state)
      go(attn_fwd_kernel<T, TD, 64, 1, P.vpath, P.subt, P.nt, P.nbuf, P.kreg,
                         0, ba_seg_args>);
    else
      go(attn_fwd_kernel<T, TD, 64, 0, P.vpath, P.subt, P.nt, P.nbuf, P.kreg,
                         0, ba_seg_args>);
    return ba_launch_status();
  });
}

// ---- band form ------------------------------------------------------------
// What a *_band entry point adds to the plain call: the band as given.
struct fwd_band_call {
  int64_t lo, hi;
};

// The band a kernel gets: lo > hi is the caller's bug; causal cuts the band
// at the diagonal (the band kernels never read `causal`); the bounds are
// clamped so that no row difference can overflow against them.
static int ba_band_for_kernel(int64_t lo, int64_t hi, int causal,
                              ba_band_args* out) {
  if (lo > hi)
    return ba_fail(BAHIP_ERR_BAND, "band: lo=%lld is above hi=%lld",
                   (long long)lo, (long long)hi);
  if (causal && lo < 0) lo = 0;
  out->lo = ba_band_clamp(lo);
  out->hi = ba_band_clamp(hi);
  return 0;
}

// The forward with a band: as with ids, the default variant only, V
// transposed in the kernel (the V^T workspace is ignored), never the module
// kernel.  No pre-pass: the kernel computes its tile range itself.
static int fwd_band_entry(const fwd_args& a, const fwd_band_call& bc,
                          int out_state, int64_t B, int64_t Sq, int64_t Sk,
                          int64_t D, int dtype, hipStream_t stream) {
  ba_band_args bd;
  if (int rc = ba_band_for_kernel(bc.lo, bc.hi, a.causal, &bd)) return rc;
  if (int rc = fwd_default_variant_only("a band")) return rc;
  if (B < 1 || B > 65535 || Sq < 1 || Sk < 1)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "band: unsupported shape B=%d Sq=%d Sk=%d", (int)B, (int)Sq,
                   (int)Sk);
  return ba_dispatch_td(D, dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    constexpr int TD = decltype(td)::D;
    constexpr ba_fwd_variant P = BA_FWD_PRODUCTION;
    const dim3 grid = fwd_grid(a, B, P.nt);
    auto go = [&](auto kernel) {
      kernel<<<grid, dim3(P.nt), 0, stream>>>(
          (const T*)a.q, (const T*)a.k, (const T*)a.v, a.o, a.lse, a.Sq, a.Sk,
          a.N, a.G, a.q_sb, a.q_ss, a.q_sh, a.k_sb, a.k_ss, a.k_sh, a.v_sb,
          a.v_ss, a.v_sh, a.scale, a.causal, a.st_acc, a.st_m, a.st_l, a.a_sb,
          a.a_ss, a.a_sh, a.ml_sb, a.ml_sh, a.carry_in, bd);
    };
    if (out_state)
      go(attn_fwd_kernel<T, TD, 64, 1, P.vpath, P.subt, P.nt, P.nbuf, P.kreg,
                         0, ba_band_args>);
    else
      go(attn_fwd_kernel<T, TD, 64, 0, P.vpath, P.subt, P.nt, P.nbuf, P.kreg,
                         0, ba_band_args>);
    return ba_launch_status();
  });
}

// The per-call knobs: the variant the BA_FWD_* table selects, and whether
// a call with these shapes stages V from the V^T image (vt_image.h).
// BA_FWD_VT=1 forces the image wherever the default variant runs, 0 forces
// the in-kernel transpose, unset applies the auto rule; an experiment
// variant always transposes in the kernel.
static int fwd_read_knobs(int64_t Sq, int64_t G, ba_fwd_choice* c,
                          bool* use_vt) {
  ba_fwd_knobs kn;
  kn.vpath = ba_env_int(BA_FWD_KNOB_SPECS[0].env, kn.vpath);
  kn.subt = ba_env_int(BA_FWD_KNOB_SPECS[1].env, kn.subt);
  kn.nt = ba_env_int(BA_FWD_KNOB_SPECS[2].env, kn.nt);
  kn.nbuf = ba_env_int(BA_FWD_KNOB_SPECS[3].env, kn.nbuf);
  kn.kreg = ba_env_int(BA_FWD_KNOB_SPECS[4].env, kn.kreg);
  *c = ba_fwd_select(kn);
  if (c->bad_knob)
    return ba_fail(BAHIP_ERR_BAD_KNOB, "%s=%d is not an accepted value",
                   c->bad_knob, c->bad_value);
  const char* e = getenv("BA_FWD_VT");
  const int vt = e ? e[0] - '0' : -1;  // "0" or "1", nothing else
  if (e && !((vt == 0 || vt == 1) && e[1] == '\0'))
    return ba_fail(BAHIP_ERR_BAD_KNOB, "BA_FWD_VT=%s is not an accepted value",
                   e);
  *use_vt = c->variant == BA_FWD_PRODUCTION &&
            (vt < 0 ? ba_vt_reuse(Sq, G) >= BA_VT_AUTO_MIN_REUSE : vt == 1);
  return 0;
}

// the pre-pass: img (capacity img_bytes) <- V^T image of v
static int vt_image_entry(const void* v, void* img, int64_t img_bytes,
                          int64_t B, int64_t Sk, int64_t Nk, int64_t D,
                          const int64_t* vs, int dtype, void* stream) {
  if (B < 1 || Sk < 1 || Nk < 1 || Nk > 65535 || B > 65535)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "V^T image: unsupported shape B=%d Sk=%d Nk=%d", (int)B,
                   (int)Sk, (int)Nk);
  if (!img || !ba_vt_workspace_fits(img_bytes, B, Nk, Sk, D))
    return ba_fail(BAHIP_ERR_WORKSPACE,
                   "V^T image workspace of %lld bytes is smaller than the "
                   "%lld needed",
                   (long long)img_bytes, (long long)ba_vt_bytes(B, Nk, Sk, D));
  const dim3 grid((unsigned)ba_vt_tiles(Sk), (unsigned)Nk, (unsigned)B);
  return ba_dispatch_td(D, dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    attn_vt_image_kernel<T, decltype(td)::D>
        <<<grid, 256, 0, (hipStream_t)stream>>>(
            (const T*)v, (T*)img, (int)Sk, (int)Nk, vs[0], vs[1], vs[2],
            img_bytes / (int64_t)sizeof(T));
    return ba_launch_status();
  });
}

// Shared body of every forward entry point (Nk = N for the equal-heads
// symbols; the kernel gets the group size G = N / Nk).  out_state = 0: the
// stateless tile (o, lse; state pointers null).  out_state = 1: the
// carry-in accumulator (o/lse null), launched through hip_function when
// one is given, else through the variant the BA_FWD_* knobs select.
// ws / ws_bytes: workspace for the V^T image, or null: with one, a call the
// knobs route to the image form runs the pre-pass and then the forward on
// the same stream; without one every call transposes in the kernel.
static int fwd_entry(void* hip_function, int out_state, const void* q,
                     const void* k, const void* v, float* o, float* lse,
                     int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk,
                     int64_t D, const int64_t* qs, const int64_t* ks,
                     const int64_t* vs, float scale, int causal, int dtype,
                     float* acc, float* m,
                     float* l, const int64_t* as, const int64_t* mls,
                     int carry_in, void* ws, int64_t ws_bytes, void* stream,
                     const fwd_seg_call* seg = nullptr,
                     const fwd_band_call* band = nullptr) {
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
  static const int64_t none[3] = {0, 0, 0};
  if (!out_state) as = mls = none;
  const fwd_args a = {q, k, v, o, lse, (int)Sq, (int)Sk, (int)N, (int)G,
                      qs[0], qs[1], qs[2], ks[0], ks[1], ks[2],
                      vs[0], vs[1], vs[2], scale, causal, acc, m, l,
                      as[0], as[1], as[2], mls[0], mls[1], carry_in};
  if (seg)
    return fwd_seg_entry(a, *seg, out_state, B, Sq, Sk, D, dtype,
                         (hipStream_t)stream);
  if (band)
    return fwd_band_entry(a, *band, out_state, B, Sq, Sk, D, dtype,
                          (hipStream_t)stream);
  if (hip_function) {
    if (D != 128 || (dtype != BAHIP_F16 && dtype != BAHIP_BF16))
      return ba_fail(BAHIP_ERR_UNSUPPORTED,
                     "module forward: unsupported head_dim %d / dtype %d",
                     (int)D, dtype);
    size_t size = sizeof a;
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, (void*)&a,
                   HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    const dim3 grid = fwd_grid(a, B, BA_FWD_PRODUCTION.nt);
    hipError_t e = hipModuleLaunchKernel(
        (hipFunction_t)hip_function, grid.x, grid.y, grid.z,
        BA_FWD_PRODUCTION.nt, 1, 1, 0, (hipStream_t)stream, nullptr, cfg);
    if (e != hipSuccess)
      return ba_fail((int)e, "module forward launch failed: %s",
                     hipGetErrorString(e));
    return ba_ok();
  }
  ba_fwd_choice c;
  bool use_vt;
  if (int rc = fwd_read_knobs(Sq, G, &c, &use_vt)) return rc;
  if (use_vt && ws) {
    if (int rc = vt_image_entry(v, ws, ws_bytes, B, Sk, Nk, D, vs, dtype,
                                stream))
      return rc;
    // same kernarg list: v is the image, v_sb / v_sh its strides
    fwd_args ai = a;
    ai.v = ws;
    ai.v_sb = ba_vt_batch_stride(Nk, Sk, D);
    ai.v_ss = 0;
    ai.v_sh = ba_vt_head_stride(Sk, D);
    return ba_dispatch_td(D, dtype, [&](auto td) {
      using T = typename decltype(td)::type;
      constexpr int TD = decltype(td)::D;
      constexpr ba_fwd_variant P = BA_FWD_PRODUCTION;
      if (out_state)
        launch_fwd<T, TD, 1, P.vpath, P.subt, P.nt, P.nbuf, P.kreg, 1>(
            ai, B, (hipStream_t)stream);
      else
        launch_fwd<T, TD, 0, P.vpath, P.subt, P.nt, P.nbuf, P.kreg, 1>(
            ai, B, (hipStream_t)stream);
      return ba_launch_status();
    });
  }
  return ba_dispatch_td(D, dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    constexpr int TD = decltype(td)::D;
#define BA_FWD_CASE(VP, ST, NTV, NB, KR)                                   \
  if (c.variant == ba_fwd_variant{VP, ST, NTV, NB, KR}) {                  \
    if (out_state)                                                         \
      launch_fwd<T, TD, 1, VP, ST, NTV, NB, KR>(a, B, (hipStream_t)stream); \
    else                                                                   \
      launch_fwd<T, TD, 0, VP, ST, NTV, NB, KR>(a, B, (hipStream_t)stream); \
  }
    BA_FWD_VARIANTS(BA_FWD_CASE)
#undef BA_FWD_CASE
    return ba_launch_status();
  });
}

extern "C" int bahip_attn_fwd_gqa(
    const void* q, const void* k, const void* v, float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    void* stream) {
  return fwd_entry(nullptr, 0, q, k, v, o, lse, B, Sq, Sk, N, Nk, D, q_strides,
                   k_strides, v_strides, softmax_scale, causal, dtype, nullptr,
                   nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, stream);
}

extern "C" int bahip_attn_fwd_gqa_ws(
    const void* q, const void* k, const void* v, float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    void* workspace, int64_t workspace_bytes, void* stream) {
  return fwd_entry(nullptr, 0, q, k, v, o, lse, B, Sq, Sk, N, Nk, D, q_strides,
                   k_strides, v_strides, softmax_scale, causal, dtype, nullptr,
                   nullptr, nullptr, nullptr, nullptr, 0, workspace,
                   workspace_bytes, stream);
}

extern "C" int bahip_attn_fwd_accum_gqa_ws(
    void* hip_function, const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in, void* workspace,
    int64_t workspace_bytes, void* stream) {
  return fwd_entry(hip_function, 1, q, k, v, nullptr, nullptr, B, Sq, Sk, N,
                   Nk, D, q_strides, k_strides, v_strides, softmax_scale,
                   causal, dtype, acc, m, l, acc_strides, ml_strides, carry_in,
                   workspace, workspace_bytes, stream);
}

extern "C" int bahip_attn_fwd_seg(
    const void* q, const void* k, const void* v, float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    void* workspace, int64_t workspace_bytes, const int32_t* q_seg,
    const int32_t* kv_seg, int64_t q_seg_stride, int64_t kv_seg_stride,
    void* seg_workspace, int64_t seg_workspace_bytes, void* stream) {
  int given;
  if (int rc = seg_ids_given(q_seg, kv_seg, &given)) return rc;
  const fwd_seg_call sc = {q_seg, kv_seg, q_seg_stride, kv_seg_stride,
                           seg_workspace, seg_workspace_bytes};
  return fwd_entry(nullptr, 0, q, k, v, o, lse, B, Sq, Sk, N, Nk, D, q_strides,
                   k_strides, v_strides, softmax_scale, causal, dtype, nullptr,
                   nullptr, nullptr, nullptr, nullptr, 0, workspace,
                   workspace_bytes, stream, given ? &sc : nullptr);
}

extern "C" int bahip_attn_fwd_accum_seg(
    void* hip_function, const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in, void* workspace,
    int64_t workspace_bytes, const int32_t* q_seg, const int32_t* kv_seg,
    int64_t q_seg_stride, int64_t kv_seg_stride, void* seg_workspace,
    int64_t seg_workspace_bytes, void* stream) {
  int given;
  if (int rc = seg_ids_given(q_seg, kv_seg, &given)) return rc;
  const fwd_seg_call sc = {q_seg, kv_seg, q_seg_stride, kv_seg_stride,
                           seg_workspace, seg_workspace_bytes};
  return fwd_entry(hip_function, 1, q, k, v, nullptr, nullptr, B, Sq, Sk, N,
                   Nk, D, q_strides, k_strides, v_strides, softmax_scale,
                   causal, dtype, acc, m, l, acc_strides, ml_strides, carry_in,
                   workspace, workspace_bytes, stream, given ? &sc : nullptr);
}

extern "C" int bahip_attn_fwd_band(
    const void* q, const void* k, const void* v, float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    int64_t band_lo, int64_t band_hi, void* stream) {
  const fwd_band_call bc = {band_lo, band_hi};
  return fwd_entry(nullptr, 0, q, k, v, o, lse, B, Sq, Sk, N, Nk, D, q_strides,
                   k_strides, v_strides, softmax_scale, causal, dtype, nullptr,
                   nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, stream,
                   nullptr, &bc);
}

extern "C" int bahip_attn_fwd_accum_band(
    void* hip_function, const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in, int64_t band_lo,
    int64_t band_hi, void* stream) {
  const fwd_band_call bc = {band_lo, band_hi};
  return fwd_entry(hip_function, 1, q, k, v, nullptr, nullptr, B, Sq, Sk, N,
                   Nk, D, q_strides, k_strides, v_strides, softmax_scale,
                   causal, dtype, acc, m, l, acc_strides, ml_strides, carry_in,
                   nullptr, 0, stream, nullptr, &bc);
}

extern "C" int bahip_attn_fwd_state_init(
    float* acc, float* m, float* l, int64_t B, int64_t S, int64_t N, int64_t D,
    const int64_t acc_strides[3], const int64_t ml_strides[2], void* stream) {
  if (B < 1 || B > 65535 || S < 1 || N < 1 || (D != 64 && D != 128))
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "state init: unsupported shape B=%d S=%d N=%d D=%d", (int)B,
                   (int)S, (int)N, (int)D);
  const bool vec = (uintptr_t)acc % 16 == 0 && acc_strides[0] % 4 == 0 &&
                   acc_strides[1] % 4 == 0 && acc_strides[2] % 4 == 0;
  const int64_t threads = S * N * (vec ? D / 4 : D);
  const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)B);
  auto go = [&](auto kernel) {
    kernel<<<grid, 256, 0, (hipStream_t)stream>>>(
        acc, m, l, (int)S, (int)N, (int)D, acc_strides[0], acc_strides[1],
        acc_strides[2], ml_strides[0], ml_strides[1]);
  };
  if (vec)
    go(attn_fwd_state_init_kernel<4>);
  else
    go(attn_fwd_state_init_kernel<1>);
  return ba_launch_status();
}

extern "C" int64_t bahip_attn_seg_workspace_bytes(int64_t B, int64_t Sq,
                                                  int64_t Sk) {
  return ba_seg_ws_bytes(B, Sq, Sk);
}

extern "C" int bahip_attn_seg_prepass(const int32_t* q_seg,
                                      const int32_t* kv_seg,
                                      int64_t q_seg_stride,
                                      int64_t kv_seg_stride, int64_t B,
                                      int64_t Sq, int64_t Sk,
                                      void* seg_workspace,
                                      int64_t seg_workspace_bytes,
                                      void* stream) {
  if (!q_seg || !kv_seg || B < 1 || B > 65535 || Sq < 1 || Sk < 1)
    return ba_fail(BAHIP_ERR_UNSUPPORTED,
                   "segment pre-pass: ids null or unsupported shape B=%d "
                   "Sq=%d Sk=%d",
                   (int)B, (int)Sq, (int)Sk);
  if (!seg_workspace || seg_workspace_bytes < ba_seg_ws_bytes(B, Sq, Sk))
    return ba_fail(BAHIP_ERR_WORKSPACE,
                   "segment workspace of %lld bytes is smaller than the %lld "
                   "needed",
                   (long long)(seg_workspace ? seg_workspace_bytes : 0),
                   (long long)ba_seg_ws_bytes(B, Sq, Sk));
  const ba_seg_ws_layout w = ba_seg_ws(B, Sq, Sk);
  int32_t* ws = (int32_t*)seg_workspace;
  if (int rc = ba_seg_prepass(q_seg, q_seg_stride, Sq, kv_seg, kv_seg_stride,
                              Sk, B, ws + w.flags_kv, ws + w.kv_tile_mm,
                              ws + w.q_blk_range, (hipStream_t)stream))
    return rc;
  return ba_seg_prepass(kv_seg, kv_seg_stride, Sk, q_seg, q_seg_stride, Sq, B,
                        ws + w.flags_q, ws + w.q_tile_mm, ws + w.kv_blk_range,
                        (hipStream_t)stream);
}

extern "C" int64_t bahip_attn_vt_image_bytes(int64_t B, int64_t Nk,
                                             int64_t Sk, int64_t D) {
  return ba_vt_bytes(B, Nk, Sk, D);
}

extern "C" int64_t bahip_attn_fwd_workspace_bytes(int64_t B, int64_t Sq,
                                                  int64_t Sk, int64_t N,
                                                  int64_t Nk, int64_t D) {
  ba_fwd_choice c;
  bool use_vt;
  const int64_t G = ba_gqa_group(N, Nk);
  // a bad knob or head pair is reported by the forward call itself
  if (!G || fwd_read_knobs(Sq, G, &c, &use_vt) || !use_vt) return 0;
  return ba_vt_bytes(B, Nk, Sk, D);
}

extern "C" int bahip_attn_vt_image(const void* v, void* image,
                                   int64_t image_bytes, int64_t B, int64_t Sk,
                                   int64_t Nk, int64_t D,
                                   const int64_t v_strides[3], int dtype,
                                   void* stream) {
  return vt_image_entry(v, image, image_bytes, B, Sk, Nk, D, v_strides, dtype,
                        stream);
}

extern "C" int bahip_attn_fwd_accum_gqa(
    void* hip_function, const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in, void* stream) {
  return fwd_entry(hip_function, 1, q, k, v, nullptr, nullptr, B, Sq, Sk, N,
                   Nk, D, q_strides, k_strides, v_strides, softmax_scale,
                   causal, dtype, acc, m, l, acc_strides, ml_strides, carry_in,
                   nullptr, 0, stream);
}

// the equal-heads symbols: Nk = N
extern "C" int bahip_attn_fwd(const void* q, const void* k, const void* v,
                              float* o, float* lse, int64_t B, int64_t Sq,
                              int64_t Sk, int64_t N, int64_t D,
                              const int64_t q_strides[3],
                              const int64_t k_strides[3],
                              const int64_t v_strides[3], float softmax_scale,
                              int causal, int dtype, void* stream) {
  return bahip_attn_fwd_gqa(q, k, v, o, lse, B, Sq, Sk, N, N, D, q_strides,
                            k_strides, v_strides, softmax_scale, causal, dtype,
                            stream);
}

extern "C" int bahip_attn_fwd_accum(
    const void* q, const void* k, const void* v, int64_t B, int64_t Sq,
    int64_t Sk, int64_t N, int64_t D, const int64_t q_strides[3],
    const int64_t k_strides[3], const int64_t v_strides[3],
    float softmax_scale, int causal, int dtype, float* acc, float* m,
    float* l, const int64_t acc_strides[3], const int64_t ml_strides[2],
    int carry_in, void* stream) {
  return bahip_attn_fwd_accum_gqa(nullptr, q, k, v, B, Sq, Sk, N, N, D,
                                  q_strides, k_strides, v_strides,
                                  softmax_scale, causal, dtype, acc, m, l,
                                  acc_strides, ml_strides, carry_in, stream);
}

extern "C" int bahip_attn_fwd_accum_fn(
    void* hip_function, const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in, void* stream) {
  return bahip_attn_fwd_accum_gqa(hip_function, q, k, v, B, Sq, Sk, N, N, D,
                                  q_strides, k_strides, v_strides,
                                  softmax_scale, causal, dtype, acc, m, l,
                                  acc_strides, ml_strides, carry_in, stream);
}

extern "C" int bahip_attn_fwd_finalize(const float* acc, const float* m,
                                       const float* l, void* o, float* lse,
                                       int64_t B, int64_t S, int64_t N,
                                       int64_t D, int dtype, void* stream) {
  const int rows_per_block = (D == 64) ? 64 : 32;  // 4 waves x 64/(D/16)
  dim3 grid((unsigned)((S + rows_per_block - 1) / rows_per_block), (unsigned)N,
            (unsigned)B);
  return ba_dispatch_td(D, dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    attn_fwd_finalize_kernel<T, decltype(td)::D>
        <<<grid, 256, 0, (hipStream_t)stream>>>(acc, m, l, (T*)o, lse, (int)S,
                                                (int)N);
    return ba_launch_status();
  });
}
