// Block-sparse forward of the D = 64/128 tile kernels, and the pre-pass that
// turns a block mask into tile lists.
//
// The kernel is attn_fwd_kernel of attn_fwd.hip in its block form (one
// ba_blk_args in the trailing pack): an indexed tile stream, described above
// that template.  Its instantiations live in this translation unit so that
// they are built without packed fp32 VALU ops (the per-source flags of
// build_ext.py), while attn_fwd.hip keeps its flags and its generated code.

#define BA_KERNELS_ONLY
#include "attn_fwd.hip"

namespace {

// Pre-pass (rule and layout: blk_support.h).  One workgroup per (own block,
// mask head, mask batch row); thread i of a pass looks at streamed tile
// 256 * pass + i, ORs the workgroup's eight waves into the tile's wave mask,
// and the surviving tiles are compacted in ascending order: a ballot and its
// prefix count within each wave, the four waves' totals through LDS.  No
// atomics, so the list is the same in every run.
__global__ __launch_bounds__(256) void blk_list_kernel(
    const uint8_t* __restrict__ mask, int64_t s_b, int64_t s_h, int64_t s_own,
    int64_t s_str, int log2_bs, int S_own, int S_str, int causal, int own_is_q,
    int32_t* __restrict__ cnt, uint32_t* __restrict__ list, int stride) {
  __shared__ int wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int blk = blockIdx.x, hm = blockIdx.y, bm = blockIdx.z;
  const ba_blk_plane p = {mask + bm * s_b + hm * s_h, s_own, s_str, log2_bs};
  const int64_t li = ((int64_t)bm * gridDim.y + hm) * gridDim.x + blk;
  uint32_t* out = list + li * stride;
  const int ntiles = (int)ba_blk_tiles(S_str);  // <= stride
  int base = 0;
  for (int t0 = 0; t0 < ntiles; t0 += 256) {
    const int t = t0 + tid;
    const uint32_t wm =
        t < ntiles ? ba_blk_wave_mask(p, blk, t, S_own, S_str, causal != 0,
                                      own_is_q != 0)
                   : 0u;
    const unsigned long long bal = __ballot(wm != 0);
    const int pre = __popcll(bal & ((1ull << lane) - 1));
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int off = base, total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < w) off += wsum[i];
      total += wsum[i];
    }
    if (wm) out[off + pre] = ba_blk_entry(t, wm);
    base += total;
    __syncthreads();  // wsum is rewritten by the next pass
  }
  if (tid == 0) cnt[li] = base;
}

}  // namespace

int ba_blk_prepass(const ba_blk_call& c, int64_t Sq, int64_t Sk, int causal,
                   bool q_side, bool kv_side, hipStream_t stream) {
  const ba_blk_ws_layout w = ba_blk_ws(c.Bm, c.Hm, Sq, Sk);
  uint32_t* ws = (uint32_t*)c.ws;
  if (q_side)
    blk_list_kernel<<<dim3((unsigned)ba_blk_blocks(Sq), (unsigned)c.Hm,
                           (unsigned)c.Bm),
                      256, 0, stream>>>(
        c.mask, c.ms[0], c.ms[1], c.ms[2], c.ms[3], c.log2_bs, (int)Sq,
        (int)Sk, causal, 1, (int32_t*)(ws + w.q_cnt), ws + w.q_list,
        (int)ba_blk_tiles(Sk));
  if (kv_side)
    blk_list_kernel<<<dim3((unsigned)ba_blk_blocks(Sk), (unsigned)c.Hm,
                           (unsigned)c.Bm),
                      256, 0, stream>>>(
        c.mask, c.ms[0], c.ms[1], c.ms[3], c.ms[2], c.log2_bs, (int)Sk,
        (int)Sq, causal, 0, (int32_t*)(ws + w.kv_cnt), ws + w.kv_list,
        (int)ba_blk_tiles(Sq));
  return ba_launch_status();
}

// Pre-pass of the q side, then the forward, on the same stream.
int ba_blk_fwd(const fwd_args& a, const ba_blk_call& c, int out_state,
               int64_t B, int64_t D, int dtype, hipStream_t stream) {
  if (int rc = ba_blk_prepass(c, a.Sq, a.Sk, a.causal, true, false, stream))
    return rc;
  const ba_blk_ws_layout w = ba_blk_ws(c.Bm, c.Hm, a.Sq, a.Sk);
  const uint32_t* ws = (const uint32_t*)c.ws;
  const ba_blk_args ba = {ws + w.q_list, (const int32_t*)(ws + w.q_cnt),
                          (int)ba_blk_tiles(a.Sk), (int)c.Hm,
                          c.Bm > 1 ? 1 : 0, c.Hm > 1 ? 1 : 0};
  return ba_dispatch_td(D, dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    constexpr int TD = decltype(td)::D;
    constexpr ba_fwd_variant P = BA_FWD_PRODUCTION;
    // wave w of a workgroup owns 32 q rows: P.nt threads cover P.nt / 2
    const dim3 grid((unsigned)((a.Sq + P.nt / 2 - 1) / (P.nt / 2)),
                    (unsigned)a.N, (unsigned)B);
    auto go = [&](auto kernel) {
      kernel<<<grid, dim3(P.nt), 0, stream>>>(
          (const T*)a.q, (const T*)a.k, (const T*)a.v, a.o, a.lse, a.Sq, a.Sk,
          a.N, a.G, a.q_sb, a.q_ss, a.q_sh, a.k_sb, a.k_ss, a.k_sh, a.v_sb,
          a.v_ss, a.v_sh, a.scale, a.causal, a.st_acc, a.st_m, a.st_l, a.a_sb,
          a.a_ss, a.a_sh, a.ml_sb, a.ml_sh, a.carry_in, ba);
    };
    if (out_state)
      go(attn_fwd_kernel<T, TD, 64, 1, P.vpath, P.subt, P.nt, P.nbuf, P.kreg,
                         0, ba_blk_args>);
    else
      go(attn_fwd_kernel<T, TD, 64, 0, P.vpath, P.subt, P.nt, P.nbuf, P.kreg,
                         0, ba_blk_args>);
    return ba_launch_status();
  });
}
