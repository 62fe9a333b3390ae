// Soft-capped backward of the D = 64/128 tile kernels.
//
// The kernels are bwd_dq_kernel and bwd_dkv_kernel of attn_bwd.hip in their
// cap form (one ba_cap_args in the trailing pack): the default plan's dq
// kernel and the split dV / dK kernels, with and without the GQA loop, in the
// plan's order, so the backward stays bitwise run-to-run identical.  Their
// instantiations live in this translation unit so that they are built without
// packed fp32 VALU ops (the per-source flags of build_ext.py), while
// attn_bwd.hip keeps the flags and the generated code of its tuned kernels.

#define BA_KERNELS_ONLY
#include "attn_bwd.hip"

namespace {

template <typename T, typename K>
void launch_cap(K kernel, dim3 grid, const bwd_dq_args& a,
                const ba_cap_args& cp, hipStream_t stream) {
  kernel<<<grid, 512, 0, stream>>>(
      (const T*)a.dout, (const T*)a.q, (const T*)a.k, (const T*)a.v, a.delta,
      a.lse, a.out, a.Sq, a.Sk, a.N, a.G, a.g_sb, a.g_ss, a.g_sh, a.q_sb,
      a.q_ss, a.q_sh, a.k_sb, a.k_ss, a.k_sh, a.v_sb, a.v_ss, a.v_sh, a.d_sb,
      a.d_sh, a.l_sb, a.l_sh, a.o_sb, a.o_ss, a.o_sh, a.scale, a.causal, cp);
}

// one workgroup column per KV head; G > 1 runs the group-loop (GQA = 1) form
template <typename T, int D, int MODE>
void launch_dkv_cap(const bwd_dq_args& a, const ba_cap_args& cp, int64_t B,
                    hipStream_t stream) {
  const dim3 grid((unsigned)((a.Sk + 255) / 256), (unsigned)(a.N / a.G),
                  (unsigned)B);
  if (a.G > 1)
    launch_cap<T>(bwd_dkv_kernel<T, D, MODE, 64, 1, ba_cap_args>, grid, a, cp,
                  stream);
  else
    launch_cap<T>(bwd_dkv_kernel<T, D, MODE, 64, 0, ba_cap_args>, grid, a, cp,
                  stream);
}

}  // namespace

int ba_cap_bwd(const bwd_dq_args& dq, const bwd_dq_args& dv,
               const bwd_dq_args& dk, const ba_cap_args& cp, int64_t B,
               int64_t D, int dtype, hipStream_t stream) {
  return ba_dispatch_td(D, dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    constexpr int TD = decltype(td)::D;
    const dim3 qgrid((unsigned)((dq.Sq + 255) / 256), (unsigned)dq.N,
                     (unsigned)B);
    launch_cap<T>(bwd_dq_kernel<T, TD, 0, ba_cap_args>, qgrid, dq, cp, stream);
    BA_CHECK_LAUNCH();
    launch_dkv_cap<T, TD, 0>(dv, cp, B, stream);
    BA_CHECK_LAUNCH();
    launch_dkv_cap<T, TD, 1>(dk, cp, B, stream);
    return ba_launch_status();
  });
}
