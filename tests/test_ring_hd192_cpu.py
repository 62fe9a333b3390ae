"""q/k head_dim 192 with v head_dim 128 through the ring on CPU (gloo).

The ring carries k and v as separate tensors and sizes every o-shaped buffer
by what it is handed, so with a two-width tile provider injected (fp32 math
of its own, independent of ``oracle.tile_fwd``) the zigzag and striped
rings at W = 2 and the 2 x 2 double ring match eager fp64 attention.  Also
pins what the interface refuses for this shape before any round, and that
any other pair of differing widths keeps its message.
"""

import math

import numpy as np
import pytest
import torch
import torch.distributed as dist

from oracle.partition import get_chunk

from .cpu_tile_provider import OracleTileProvider
from .gloo_ranks import run_ranks
from .test_ring_cpu import ATOL, RTOL

DQK, DV = 192, 128


def _scores(q, k, scale, causal):
    ke = k.float().repeat_interleave(q.shape[2] // k.shape[2], dim=2)
    s = torch.einsum("bqnd,bknd->bnqk", q.float(), ke) * scale
    if causal:
        s = s.masked_fill(~torch.ones(s.shape[-2:], dtype=torch.bool).tril(),
                          -math.inf)
    return s, ke


class TwoWidthTileProvider(OracleTileProvider):
    """The oracle provider's state and merge with fp32 tile math that takes
    o's width from v."""

    def fwd(self, q, k, v, scale, causal):
        s, _ = _scores(q, k, scale, causal)
        ve = v.float().repeat_interleave(q.shape[2] // v.shape[2], dim=2)
        o = torch.einsum("bnqk,bknd->bqnd", torch.softmax(s, -1), ve)
        return o.contiguous(), torch.logsumexp(s, -1)

    def bwd(self, do, q, k, v, delta, lse, scale, causal, deterministic):
        g, nk = q.shape[2] // k.shape[2], k.shape[2]
        s, ke = _scores(q, k, scale, causal)
        ve = v.float().repeat_interleave(g, dim=2)
        p = torch.exp(s - lse.unsqueeze(-1))
        dp = torch.einsum("bqnd,bknd->bnqk", do.float(), ve)
        ds = p * (dp - delta.unsqueeze(-1)) * scale
        dq = torch.einsum("bnqk,bknd->bqnd", ds, ke)
        dk = torch.einsum("bnqk,bqnd->bknd", ds, q.float())
        dv = torch.einsum("bnqk,bqnd->bknd", p, do.float())
        fold = lambda t: t.reshape(*t.shape[:2], nk, g, t.shape[3]).sum(3)
        return dq, fold(dk), fold(dv)

    def fwd_accum(self, state, q, k, v, scale, causal, row_offset=0):
        import oracle

        o_i, lse_i = self.fwd(q, k, v, scale, causal)
        if state is None:
            assert row_offset == 0
            return [o_i, lse_i.transpose(-2, -1).unsqueeze(-1).contiguous()]
        o, lse = state
        sl = slice(row_offset, row_offset + q.shape[1])
        o[:, sl], lse[:, sl] = oracle.scale_out_lse(o[:, sl], lse[:, sl], o_i,
                                                    lse_i)
        return state


def _reference(q, k, v, do, causal):
    """(o, dq, dk, dv) of eager attention in fp64, scale 1/sqrt(192)."""
    q, k, v = (t.double().requires_grad_() for t in (q, k, v))
    g = q.shape[2] // k.shape[2]
    ke, ve = (t.repeat_interleave(g, dim=2) for t in (k, v))
    s = torch.einsum("bqnd,bknd->bnqk", q, ke) / math.sqrt(DQK)
    if causal:
        s = s.masked_fill(~torch.ones(s.shape[-2:], dtype=torch.bool).tril(),
                          -math.inf)
    o = torch.einsum("bnqk,bknd->bqnd", torch.softmax(s, -1), ve)
    return tuple(t.detach().float()
                 for t in (o, *torch.autograd.grad(o, (q, k, v), do.double())))


def _worker(rank, world, causal, striped, optimize_bwd_comm, local):
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped
    from burst_attn_amd.tile import _set_tile_provider_for_testing

    _set_tile_provider_for_testing(TwoWidthTileProvider())
    double_group = [None, None]
    if local:
        ranks = np.arange(world).reshape(-1, local)
        intra = [dist.new_group(list(r)) for r in ranks]
        inter = [dist.new_group(list(r)) for r in ranks.T]
        double_group = [intra[rank // local], inter[rank % local]]
    b, s, n, nk = 1, 32 * world, 4, 2
    g = torch.Generator().manual_seed(192128)
    q, k, v, do = (torch.randn(b, s, h, d, generator=g)
                   for h, d in ((n, DQK), (nk, DQK), (nk, DV), (n, DV)))
    refs = _reference(q, k, v, do, causal)
    zig = causal and not striped
    ch = lambda t: get_chunk(t, 1, rank, world, zigzag=zig, striped=striped)
    qc, kc, vc = (ch(t).requires_grad_() for t in (q, k, v))
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(qc, kc, vc, None, "cuda", causal, optimize_bwd_comm, False, None,
             double_group)
    assert o.shape == (b, 32, n, DV)
    outs = (o, *torch.autograd.grad(o, (qc, kc, vc), ch(do)))
    for out, ref in zip(outs, refs):
        torch.testing.assert_close(out, ch(ref), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("optimize_bwd_comm", [False, True])
@pytest.mark.parametrize("striped", [False, True], ids=["zigzag", "striped"])
def test_ring_two_widths(striped, optimize_bwd_comm):
    run_ranks(_worker, 2, True, striped, optimize_bwd_comm, 0,
              what="(192, 128) ring")


def test_double_ring_two_widths():
    run_ranks(_worker, 4, True, False, True, 2, what="(192, 128) double ring")


@pytest.mark.parametrize("kw,names", [
    (dict(segment_ids=torch.zeros(1, 64, dtype=torch.int32)), "segment_ids"),
    (dict(window_size=(8, 0)), "window_size"),
    (dict(softcap=30.0), "softcap"),
    (dict(block_mask=torch.ones(1, 1, 1, 1, dtype=torch.bool)), "block_mask"),
])
def test_interface_refuses_masks(kw, names):
    from burst_attn_amd import burst_attn_func

    q, v = torch.randn(1, 64, 2, DQK), torch.randn(1, 64, 2, DV)
    with pytest.raises(ValueError, match=f"192.*128.*{names}"):
        burst_attn_func(q, q, v, None, "cuda", False, **kw)


def test_other_width_pairs_keep_their_message():
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    q, v = torch.randn(1, 32, 2, 64), torch.randn(1, 32, 2, 32)
    for func in (burst_attn_func, burst_attn_func_striped):
        with pytest.raises(ValueError, match=r"head_dim differs: q 64, k 64, "
                                             r"v 32 \(N=2, Nk=2\)"):
            func(q, q, v)
    q, k = torch.randn(1, 32, 2, DQK), torch.randn(1, 32, 2, DV)
    with pytest.raises(ValueError, match="head_dim differs: q 192, k 128"):
        burst_attn_func(q, k, k)
