"""softcap at the public interface, without a GPU: what is refused before any
round, and what the ring hands the tile provider (gloo, W=2, a recording
provider over the CPU oracle)."""

import math

import pytest
import torch

from .cpu_tile_provider import OracleTileProvider
from .gloo_ranks import run_ranks


@pytest.mark.parametrize("striped", [False, True], ids=["zigzag", "striped"])
@pytest.mark.parametrize("kw,names", [
    (dict(softcap=-1.0), "softcap"),
    (dict(softcap=math.nan), "softcap"),
    (dict(softcap="30"), "softcap"),
    (dict(softcap=1.5, segment_ids=torch.zeros(1, 32, dtype=torch.int32)),
     "softcap and segment_ids are not supported together yet"),
    (dict(softcap=1.5, window_size=(8, 0)),
     "softcap and window_size are not supported together yet"),
], ids=["negative", "nan", "string", "segment_ids", "window"])
def test_interface_refuses(kw, names, striped):
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    func = burst_attn_func_striped if striped else burst_attn_func
    q = torch.randn(1, 32, 2, 64)
    with pytest.raises(ValueError, match=names):
        func(q, q, q, None, "cuda", True, **kw)


class _Recorder(OracleTileProvider):
    """Records the keywords of every accumulate call; ``softcap`` itself is
    dropped before the oracle (which has no cap) computes the tile."""

    def __init__(self):
        self.seen = []

    def fwd_accum(self, *a, **kw):
        self.seen.append(dict(kw))
        kw.pop("softcap", None)
        return super().fwd_accum(*a, **kw)

    def bwd_accum(self, *a, **kw):
        self.seen.append(dict(kw))
        kw.pop("softcap", None)
        return super().bwd_accum(*a, **kw)


def _worker(rank, world, striped, cap):
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped
    from burst_attn_amd.tile import _set_tile_provider_for_testing

    rec = _Recorder()
    _set_tile_provider_for_testing(rec)
    g = torch.Generator().manual_seed(5 + rank)
    q, k, v = (torch.randn(1, 32, 2, 64, generator=g).requires_grad_()
               for _ in range(3))
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(q, k, v, None, "cuda", True, softcap=cap)
    grads = torch.autograd.grad(o, (q, k, v), torch.ones_like(o))
    assert all(t.shape == x.shape for t, x in zip(grads, (q, k, v)))
    assert len(rec.seen) == 2 * world  # a forward and a backward per round
    want = {"softcap": cap} if cap else {}
    for kw in rec.seen:
        assert {n: x for n, x in kw.items() if n != "row_offset"} == want, kw


@pytest.mark.parametrize("cap", [0.0, 1.5])
@pytest.mark.parametrize("striped", [False, True], ids=["zigzag", "striped"])
def test_ring_hands_the_provider_the_cap_only_when_positive(striped, cap):
    run_ranks(_worker, 2, striped, cap, what="softcap ring")
