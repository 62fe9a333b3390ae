"""head_dim 256 through the ring orchestration on CPU (gloo, W=2).

The ring, its windows, payload lists and comm layer carry no head_dim of
their own: with the GQA oracle provider injected (as in
tests/test_ring_gqa_cpu.py) a 256-wide ring, zigzag causal and striped,
matches eager attention.  Also pins what the interface refuses at D=256
before any ring or tile work: segment ids and a bounded window.
"""

import pytest
import torch

from oracle.partition import get_chunk

from .gloo_ranks import run_ranks
from .test_ring_cpu import ATOL, RTOL


def _worker(rank, world, striped, optimize_bwd_comm):
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped
    from burst_attn_amd.tile import _set_tile_provider_for_testing
    from .gqa_cpu_provider import GqaOracleTileProvider, gqa_full_reference

    _set_tile_provider_for_testing(GqaOracleTileProvider())
    b, s, n, nk, d = 1, 32 * world, 4, 2, 256
    g = torch.Generator().manual_seed(256)
    q, k, v, do = (torch.randn(b, s, h, d, generator=g) for h in (n, nk, nk, n))
    refs = gqa_full_reference(q, k, v, do, None, True)
    ch = lambda t: get_chunk(t, 1, rank, world, zigzag=not striped,
                             striped=striped)
    qc, kc, vc = (ch(t).requires_grad_() for t in (q, k, v))
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(qc, kc, vc, None, "cuda", True, optimize_bwd_comm, False)
    outs = (o, *torch.autograd.grad(o, (qc, kc, vc), ch(do)))
    for out, ref in zip(outs, refs):
        torch.testing.assert_close(out, ch(ref), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("optimize_bwd_comm", [False, True])
@pytest.mark.parametrize("striped", [False, True], ids=["zigzag", "striped"])
def test_ring_is_head_dim_generic(striped, optimize_bwd_comm):
    run_ranks(_worker, 2, striped, optimize_bwd_comm, what="D=256 ring")


@pytest.mark.parametrize("kw,names", [
    (dict(segment_ids=torch.zeros(1, 32, dtype=torch.int32)), "segment_ids"),
    (dict(window_size=(8, 0)), "window_size"),
])
def test_interface_refuses_masks_at_d256(kw, names):
    from burst_attn_amd import burst_attn_func

    q = torch.randn(1, 32, 2, 256)
    with pytest.raises(ValueError, match=f"head_dim 256.*{names}"):
        burst_attn_func(q, q, q, None, "cuda", True, **kw)
