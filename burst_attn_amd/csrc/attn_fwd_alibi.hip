// ALiBi forward of the D = 64/128 tile kernels.
//
// The kernel is attn_fwd_kernel of attn_fwd.hip in its ALiBi form (one
// ba_alibi_args in the trailing pack), stateless and carry-in.  Its
// instantiations live in this translation unit so that they are built without
// packed fp32 VALU ops (the per-source flags of build_ext.py: the bias is two
// scalar-operand FMAs per score, the second with the |.| source modifier, which
// the packed forms do not take), while attn_fwd.hip keeps the flags its tuned
// kernels were measured with and its generated code.

#define BA_KERNELS_ONLY
#include "attn_fwd.hip"

int ba_alibi_fwd(const fwd_args& a, const ba_alibi_args& al, int out_state,
                 int64_t B, int64_t D, int dtype, hipStream_t stream) {
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
          a.a_ss, a.a_sh, a.ml_sb, a.ml_sh, a.carry_in, al);
    };
    if (out_state)
      go(attn_fwd_kernel<T, TD, 64, 1, P.vpath, P.subt, P.nt, P.nbuf, P.kreg,
                         0, ba_alibi_args>);
    else
      go(attn_fwd_kernel<T, TD, 64, 0, P.vpath, P.subt, P.nt, P.nbuf, P.kreg,
                         0, ba_alibi_args>);
    return ba_launch_status();
  });
}
