// Block-sparse backward of the D = 64/128 tile kernels.
//
// The kernels are bwd_dq_kernel and bwd_dkv_kernel of attn_bwd.hip in their
// block form (one ba_blk_args in the trailing pack): the default plan's dq
// kernel on the q-owning lists and the split dV / dK kernels, with and without
// the GQA loop, on the kv-owning lists, in the plan's order, so the backward
// stays bitwise run-to-run identical.  Their instantiations live in this
// translation unit so that they are built without packed fp32 VALU ops (the
// per-source flags of build_ext.py), while attn_bwd.hip keeps its flags and
// its generated code.

#define BA_KERNELS_ONLY
#include "attn_bwd.hip"

namespace {

template <typename T, typename K>
void launch_blk(K kernel, dim3 grid, const bwd_dq_args& a,
                const ba_blk_args& ba, hipStream_t stream) {
  kernel<<<grid, 512, 0, stream>>>(
      (const T*)a.dout, (const T*)a.q, (const T*)a.k, (const T*)a.v, a.delta,
      a.lse, a.out, a.Sq, a.Sk, a.N, a.G, a.g_sb, a.g_ss, a.g_sh, a.q_sb,
      a.q_ss, a.q_sh, a.k_sb, a.k_ss, a.k_sh, a.v_sb, a.v_ss, a.v_sh, a.d_sb,
      a.d_sh, a.l_sb, a.l_sh, a.o_sb, a.o_ss, a.o_sh, a.scale, a.causal, ba);
}

// one workgroup column per KV head; G > 1 runs the group-loop (GQA = 1) form
template <typename T, int D, int MODE>
void launch_dkv_blk(const bwd_dq_args& a, const ba_blk_args& ba, int64_t B,
                    hipStream_t stream) {
  const dim3 grid((unsigned)((a.Sk + 255) / 256), (unsigned)(a.N / a.G),
                  (unsigned)B);
  if (a.G > 1)
    launch_blk<T>(bwd_dkv_kernel<T, D, MODE, 64, 1, ba_blk_args>, grid, a, ba,
                  stream);
  else
    launch_blk<T>(bwd_dkv_kernel<T, D, MODE, 64, 0, ba_blk_args>, grid, a, ba,
                  stream);
}

}  // namespace

// Pre-pass of both sides, then the three kernels, on the same stream.
int ba_blk_bwd(const bwd_dq_args& dq, const bwd_dq_args& dv,
               const bwd_dq_args& dk, const ba_blk_call& c, int64_t B,
               int64_t D, int dtype, hipStream_t stream) {
  if (int rc = ba_blk_prepass(c, dq.Sq, dq.Sk, dq.causal, true, true, stream))
    return rc;
  const ba_blk_ws_layout w = ba_blk_ws(c.Bm, c.Hm, dq.Sq, dq.Sk);
  const uint32_t* ws = (const uint32_t*)c.ws;
  const int b_mul = c.Bm > 1 ? 1 : 0, h_mul = c.Hm > 1 ? 1 : 0;
  const ba_blk_args own_q = {ws + w.q_list, (const int32_t*)(ws + w.q_cnt),
                             (int)ba_blk_tiles(dq.Sk), (int)c.Hm, b_mul, h_mul};
  const ba_blk_args own_kv = {ws + w.kv_list, (const int32_t*)(ws + w.kv_cnt),
                              (int)ba_blk_tiles(dq.Sq), (int)c.Hm, b_mul,
                              h_mul};
  return ba_dispatch_td(D, dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    constexpr int TD = decltype(td)::D;
    const dim3 qgrid((unsigned)((dq.Sq + 255) / 256), (unsigned)dq.N,
                     (unsigned)B);
    launch_blk<T>(bwd_dq_kernel<T, TD, 0, ba_blk_args>, qgrid, dq, own_q,
                  stream);
    BA_CHECK_LAUNCH();
    launch_dkv_blk<T, TD, 0>(dv, own_kv, B, stream);
    BA_CHECK_LAUNCH();
    launch_dkv_blk<T, TD, 1>(dk, own_kv, B, stream);
    return ba_launch_status();
  });
}
