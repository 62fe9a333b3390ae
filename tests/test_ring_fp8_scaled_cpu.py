"""Block-scaled FP8 (descale tensors) through the ring on CPU (gloo), zigzag
and striped at W = 2.  Every rank has scales of its own for its shard (powers
of two, so applying them is exact): dq per row, dk per 64-row tile, dv per
channel.  The injected provider dequantises with the views it is handed and
calls the oracle's forward; o matches single-process fp64 attention on the
dequantised sequence at TOL[bf16], and every call got views of the right
shapes.  The interface's refusals of malformed scale tensors need no GPU.
"""

import math

import pytest
import torch

from oracle.partition import get_chunk

from .cpu_tile_provider import OracleTileProvider
from .gloo_ranks import run_ranks
from .test_gpu_parity import TOL

FP8 = torch.float8_e4m3fn
B, S_LOCAL, N, NK, D = 1, 128, 4, 2, 128


class ScaledOracleProvider(OracleTileProvider):
    calls = 0

    def fwd_accum(self, state, q, k, v, scale, causal, row_offset=0,
                  descale=None):
        dq, dk, dv = descale
        sq, sk = q.shape[1], k.shape[1]
        assert dq.shape == (B, N, sq), dq.shape
        assert dk.shape == (B, NK, -(-sk // 64)), (dk.shape, sk)
        assert dv.shape == (B, NK, D), dv.shape
        q = q.float() * dq.transpose(1, 2)[..., None]
        k = k.float() * dk.repeat_interleave(64, 2)[:, :, :sk].transpose(
            1, 2)[..., None]
        v = v.float() * dv[:, None]
        k, v = (t.repeat_interleave(N // NK, dim=2) for t in (k, v))
        type(self).calls += 1
        return super().fwd_accum(state, q, k, v, scale, causal, row_offset)


def _pow2(g, shape, lo):
    return 2.0 ** torch.randint(lo, lo + 4, shape, generator=g).float()


def _worker(rank, world, striped):
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped
    from burst_attn_amd.tile import _set_tile_provider_for_testing

    _set_tile_provider_for_testing(ScaledOracleProvider())
    s = S_LOCAL * world
    g = torch.Generator().manual_seed(8129)
    q8, k8, v8 = (torch.randn(B, s, h, D, generator=g).to(FP8)
                  for h in (N, NK, NK))
    ch = lambda t, r=rank: get_chunk(t, 1, r, world, zigzag=not striped,
                                     striped=striped)
    # per-rank scales, scattered to the global rows that rank holds
    dq, dk, dv = ([_pow2(g, shape, lo) for _ in range(world)]
                  for shape, lo in (((B, N, S_LOCAL), -3),
                                    ((B, NK, S_LOCAL // 64), -2),
                                    ((B, NK, D), -4)))
    rows = torch.arange(s).view(1, s, 1, 1)
    qs, ks, vs = (torch.ones(B, s, h, w) for h, w in ((N, 1), (NK, 1), (NK, D)))
    for r in range(world):
        at = ch(rows, r).flatten()
        qs[:, at] = dq[r].transpose(1, 2)[..., None]
        ks[:, at] = dk[r].repeat_interleave(64, 2).transpose(1, 2)[..., None]
        vs[:, at] = dv[r][:, None].expand(B, S_LOCAL, NK, D)
    qd, kd, vd = (t.float().double() * x
                  for t, x in zip((q8, k8, v8), (qs, ks, vs)))
    ke, ve = (t.repeat_interleave(N // NK, dim=2) for t in (kd, vd))
    sc = torch.einsum("bqnd,bknd->bnqk", qd, ke) / math.sqrt(D)
    sc = sc.masked_fill(~torch.ones(s, s, dtype=torch.bool).tril(), -math.inf)
    ref = torch.einsum("bnqk,bknd->bqnd", torch.softmax(sc, -1), ve).float()
    ch8 = lambda t: ch(t.view(torch.uint8)).contiguous().view(FP8)
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(ch8(q8), ch8(k8), ch8(v8), None, "cuda", True,
             descale=(dq[rank], dk[rank], dv[rank]))
    assert o.dtype == torch.bfloat16 and ScaledOracleProvider.calls >= world
    torch.testing.assert_close(o.float(), ch(ref), **TOL[torch.bfloat16])


@pytest.mark.parametrize("striped", [False, True], ids=["zigzag", "striped"])
def test_ring_fp8_scaled(striped):
    run_ranks(_worker, 2, striped, what="scaled fp8 ring")


def _scales(s=128, **over):
    shapes = dict(dq=(1, 2, s), dk=(1, 2, -(-s // 64)), dv=(1, 2, 128))
    shapes.update(over)
    return tuple(torch.ones(shapes[n]) for n in ("dq", "dk", "dv"))


@pytest.mark.parametrize("s,descale,causal", [
    (128, _scales(dk=(1, 2, 3)), False),
    (128, _scales(dq=(1, 2, 64)), False),
    (128, tuple(t.double() for t in _scales()), False),
    (128, (_scales()[0], 1.0, 1.0), False),
    (128, (_scales()[0].requires_grad_(), *_scales()[1:]), False),
    (192, _scales(192), True),  # zigzag halves of 96 rows: not whole tiles
], ids=["dk_shape", "dq_shape", "dtype", "mixed", "grad", "s_local"])
def test_interface_refusals(s, descale, causal):
    from burst_attn_amd import burst_attn_func

    q8 = torch.zeros(1, s, 2, 128).to(FP8)
    with pytest.raises(ValueError, match="descale"):
        burst_attn_func(q8, q8, q8, None, "cuda", causal, descale=descale)
