// ALiBi backward of the D = 64/128 tile kernels.
//
// The kernels are bwd_dq_kernel and bwd_dkv_kernel of attn_bwd.hip in their
// ALiBi form (one ba_alibi_args in the trailing pack): the default plan's dq
// kernel and the split dV / dK kernels, with and without the GQA loop, in the
// plan's order and without atomics, so the backward stays bitwise run-to-run
// identical.  Their instantiations live in this translation unit for the
// reason attn_fwd_alibi.hip gives.

#define BA_KERNELS_ONLY
#include "attn_bwd.hip"

namespace {

template <typename T, typename K>
void launch_alibi(K kernel, dim3 grid, const bwd_dq_args& a,
                  const ba_alibi_args& al, hipStream_t stream) {
  kernel<<<grid, 512, 0, stream>>>(
      (const T*)a.dout, (const T*)a.q, (const T*)a.k, (const T*)a.v, a.delta,
      a.lse, a.out, a.Sq, a.Sk, a.N, a.G, a.g_sb, a.g_ss, a.g_sh, a.q_sb,
      a.q_ss, a.q_sh, a.k_sb, a.k_ss, a.k_sh, a.v_sb, a.v_ss, a.v_sh, a.d_sb,
      a.d_sh, a.l_sb, a.l_sh, a.o_sb, a.o_ss, a.o_sh, a.scale, a.causal, al);
}

// one workgroup column per KV head; G > 1 runs the group-loop (GQA = 1) form,
// which reads one slope per member of the group
template <typename T, int D, int MODE>
void launch_dkv_alibi(const bwd_dq_args& a, const ba_alibi_args& al, int64_t B,
                      hipStream_t stream) {
  const dim3 grid((unsigned)((a.Sk + 255) / 256), (unsigned)(a.N / a.G),
                  (unsigned)B);
  if (a.G > 1)
    launch_alibi<T>(bwd_dkv_kernel<T, D, MODE, 64, 1, ba_alibi_args>, grid, a,
                    al, stream);
  else
    launch_alibi<T>(bwd_dkv_kernel<T, D, MODE, 64, 0, ba_alibi_args>, grid, a,
                    al, stream);
}

}  // namespace

int ba_alibi_bwd(const bwd_dq_args& dq, const bwd_dq_args& dv,
                 const bwd_dq_args& dk, const ba_alibi_args& al, int64_t B,
                 int64_t D, int dtype, hipStream_t stream) {
  return ba_dispatch_td(D, dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    constexpr int TD = decltype(td)::D;
    const dim3 qgrid((unsigned)((dq.Sq + 255) / 256), (unsigned)dq.N,
                     (unsigned)B);
    launch_alibi<T>(bwd_dq_kernel<T, TD, 0, ba_alibi_args>, qgrid, dq, al,
                    stream);
    BA_CHECK_LAUNCH();
    launch_dkv_alibi<T, TD, 0>(dv, al, B, stream);
    BA_CHECK_LAUNCH();
    launch_dkv_alibi<T, TD, 1>(dk, al, B, stream);
    return ba_launch_status();
  });
}
