"""FP8 q/k/v through the ring on CPU (gloo): zigzag and striped at W = 2 and
the 2 x 2 double ring.  The injected provider dequantises and calls the
oracle's forward.  o is bf16 and matches single-process fp64 attention on the
dequantised inputs at TOL[bf16]; every payload on the wire is uint8; and the
interface's fp8 refusals raise without a GPU.
"""

import math

import numpy as np
import pytest
import torch
import torch.distributed as dist

from oracle.partition import get_chunk

from .cpu_tile_provider import OracleTileProvider
from .gloo_ranks import run_ranks
from .test_gpu_parity import TOL

FP8 = torch.float8_e4m3fn
DESCALE = (0.5, 0.25, 2.0)


class Fp8OracleProvider(OracleTileProvider):
    def fwd_accum(self, state, q, k, v, scale, causal, row_offset=0,
                  descale=None):
        assert q.dtype == k.dtype == v.dtype == FP8
        q, k, v = (t.float() * s for t, s in zip((q, k, v), descale))
        k, v = (t.repeat_interleave(q.shape[2] // t.shape[2], dim=2)
                for t in (k, v))
        return super().fwd_accum(state, q, k, v, scale, causal, row_offset)


def _worker(rank, world, causal, striped, local):
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped
    from burst_attn_amd.comm import Ring
    from burst_attn_amd.tile import _set_tile_provider_for_testing

    _set_tile_provider_for_testing(Fp8OracleProvider())
    wire, send = [], Ring.double_ring_send_recv

    def spy(self, payload, bufs, r):
        wire.extend(t.dtype for t in (*payload, *bufs))
        return send(self, payload, bufs, r)

    Ring.double_ring_send_recv = spy
    double_group = [None, None]
    if local:
        ranks = np.arange(world).reshape(-1, local)
        intra = [dist.new_group(list(r)) for r in ranks]
        inter = [dist.new_group(list(r)) for r in ranks.T]
        double_group = [intra[rank // local], inter[rank % local]]
    b, s, n, nk, d = 1, 32 * world, 4, 2, 128
    g = torch.Generator().manual_seed(8128)
    q8, k8, v8 = (torch.randn(b, s, h, d, generator=g).to(FP8)
                  for h in (n, nk, nk))
    qd, kd, vd = (t.float().double() * x
                  for t, x in zip((q8, k8, v8), DESCALE))
    ke, ve = (t.repeat_interleave(n // nk, dim=2) for t in (kd, vd))
    sc = torch.einsum("bqnd,bknd->bnqk", qd, ke) / math.sqrt(d)
    if causal:
        sc = sc.masked_fill(~torch.ones(s, s, dtype=torch.bool).tril(),
                            -math.inf)
    ref = torch.einsum("bnqk,bknd->bqnd", torch.softmax(sc, -1), ve).float()
    zig = causal and not striped
    ch = lambda t: get_chunk(t, 1, rank, world, zigzag=zig, striped=striped)
    ch8 = lambda t: ch(t.view(torch.uint8)).contiguous().view(FP8)
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(ch8(q8), ch8(k8), ch8(v8), None, "cuda", causal, False, False,
             None, double_group, descale=DESCALE)
    assert o.dtype == torch.bfloat16
    tol = TOL[torch.bfloat16]
    torch.testing.assert_close(o.float(), ch(ref), **tol)
    assert wire and all(t == torch.uint8 for t in wire), wire


@pytest.mark.parametrize("striped", [False, True], ids=["zigzag", "striped"])
def test_ring_fp8(striped):
    run_ranks(_worker, 2, True, striped, 0, what="fp8 ring")


def test_double_ring_fp8():
    run_ranks(_worker, 4, True, False, 2, what="fp8 double ring")


def _q8(d=128, grad=False):
    t = torch.zeros(1, 64, 2, d).to(FP8)
    return t.requires_grad_() if grad else t


@pytest.mark.parametrize("args,kw,names", [
    ((_q8(grad=True), _q8(), _q8()), {}, "require grad"),
    ((_q8(),) * 3, dict(segment_ids=torch.zeros(1, 64, dtype=torch.int32)),
     "fp8.*segment_ids"),
    ((_q8(),) * 3, dict(window_size=(8, 0)), "fp8.*window_size"),
    ((_q8(),) * 3, dict(softcap=30.0), "fp8.*softcap"),
    ((_q8(),) * 3, dict(block_mask=torch.ones(1, 1, 1, 1, dtype=torch.bool)),
     "fp8.*block_mask"),
    ((_q8(64),) * 3, {}, "fp8.*head_dim 128 only"),
    ((torch.zeros(1, 64, 2, 128),) * 3, dict(descale=(1.0, 1.0, 1.0)),
     "descale is for fp8"),
    ((_q8(),) * 3, dict(descale=(1.0, 1.0)), "descale must be"),
    ((_q8(),) * 3, dict(descale=(1.0, -1.0, 1.0)), "descale must be"),
    ((_q8(),) * 3, dict(descale=(1.0, math.inf, 1.0)), "descale must be"),
])
def test_interface_refusals(args, kw, names):
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    for func in (burst_attn_func, burst_attn_func_striped):
        if func is burst_attn_func_striped and "block_mask" in kw:
            continue  # refused for the striped op whatever the dtype
        with pytest.raises(ValueError, match=names):
            func(*args, None, "cuda", False, **kw)
