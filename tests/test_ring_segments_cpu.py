"""Segment ids through the ring orchestration on CPU (gloo).

Same structure as tests/test_ring_cpu.py with the segment-aware oracle
provider (tests/segment_cpu_provider.py) injected: every rank builds the
same packed full sequence, the reference is the dense masked softmax of
tests/segment_refs.py on the full sequence, and the rank's chunk of ids
comes from ``burst_attn_amd.local_segment_ids``.  Also pins what the ring
hands the provider: int32 ``[B, window]`` views, whose travelling side is,
from round 2 on, what came over the wire.
"""

import numpy as np
import pytest
import torch
import torch.distributed as dist

from oracle.partition import get_chunk

from .gloo_ranks import run_ranks
from .test_ring_cpu import ATOL, RTOL

B, S_LOCAL, N, NK, D = 2, 64, 4, 2, 32


def _global_cu(s):
    """Documents of mixed length: a length-1 one, boundaries on and off the
    chunk seams, one spanning more than a rank's chunk."""
    cu = [0, 1, 17, S_LOCAL // 2, S_LOCAL, S_LOCAL + 5]
    cu += [x for x in (2 * S_LOCAL + S_LOCAL // 2 + 3, 3 * S_LOCAL) if x < s]
    return cu + [s]


def _worker(rank, world, causal, striped, opt_bwd, local, id_dtype):
    from burst_attn_amd import (burst_attn_func, burst_attn_func_striped,
                                local_segment_ids, segment_ids_from_cu_seqlens)
    from burst_attn_amd.interface import get_partition_id
    from burst_attn_amd.tile import _set_tile_provider_for_testing
    from . import segment_refs as sr
    from .segment_cpu_provider import SegOracleTileProvider

    P = SegOracleTileProvider()
    _set_tile_provider_for_testing(P)
    double_group = [None, None]
    if local:
        ranks = np.arange(world).reshape(-1, local)
        intra = [dist.new_group(list(r)) for r in ranks]
        inter = [dist.new_group(list(r)) for r in ranks.T]
        double_group = [intra[rank // local], inter[rank % local]]

    s = S_LOCAL * world
    ids = segment_ids_from_cu_seqlens(_global_cu(s), s)
    ids = torch.stack([ids, ids.flip(0).max() - ids.flip(0)])  # two packings
    g = torch.Generator().manual_seed(777 + world)
    q = torch.randn(B, s, N, D, generator=g)
    k = torch.randn(B, s, NK, D, generator=g)
    v = torch.randn(B, s, NK, D, generator=g)
    do = torch.randn(B, s, N, D, generator=g)
    sc = 1.0 / D ** 0.5
    o_ref, lse_ref = sr.seg_fwd(q, k, v, sc, causal, ids, ids)
    dq_ref, dk_ref, dv_ref = sr.seg_bwd(do, q, k, v, lse_ref, sc, causal, ids,
                                        ids, o=o_ref)

    zig = causal and not striped
    layout = "striped" if striped else ("zigzag" if zig else "contiguous")
    ch = lambda t: get_chunk(t, 1, rank, world, zigzag=zig, striped=striped)
    my_ids = local_segment_ids(ids, layout, rank, world).to(id_dtype)
    qc, kc, vc = (ch(t).requires_grad_() for t in (q, k, v))
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(qc, kc, vc, None, "cuda", causal, opt_bwd, False, None,
             double_group, segment_ids=my_ids)
    dq, dk, dv = torch.autograd.grad(o, (qc, kc, vc), ch(do))
    torch.testing.assert_close(o, ch(o_ref), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(dv, ch(dv_ref), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(dk, ch(dk_ref), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(dq, ch(dq_ref), rtol=RTOL, atol=ATOL)

    # one seg per round; the travelling side (kv in the forward, q in the
    # backward) belongs to the round's source rank: after round 1 it can
    # only have come over the wire
    from burst_attn_amd.interface import tile_window
    assert len(P.fwd_segs) == world and len(P.bwd_segs) == world
    for r in range(1, world + 1):
        src = get_partition_id(double_group, r, None)
        theirs = local_segment_ids(ids, layout, src, world).to(torch.int32)
        mine = my_ids.to(torch.int32)
        qw, kw, _ = tile_window(layout if layout != "contiguous" else "zigzag",
                                rank, src, causal, S_LOCAL)
        fq, fkv = P.fwd_segs[r - 1]
        assert torch.equal(fq, mine[:, qw]) and torch.equal(fkv, theirs[:, kw])
        qw, kw, _ = tile_window(layout if layout != "contiguous" else "zigzag",
                                src, rank, causal, S_LOCAL)
        bq, bkv = P.bwd_segs[r - 1]
        assert torch.equal(bq, theirs[:, qw]) and torch.equal(bkv, mine[:, kw])


@pytest.mark.parametrize("opt_bwd", [False, True])
@pytest.mark.parametrize("causal,striped", [
    (False, False), (True, False), (True, True), (False, True)])
@pytest.mark.parametrize("world", [2, 3])
def test_segment_ring_matches_masked_attention(world, causal, striped, opt_bwd):
    run_ranks(_worker, world, causal, striped, opt_bwd, 0,
              torch.int64 if opt_bwd else torch.int32, what="segment ring")


@pytest.mark.parametrize("opt_bwd", [False, True])
@pytest.mark.parametrize("causal,striped", [
    (False, False), (True, False), (True, True), (False, True)])
def test_segment_double_ring(causal, striped, opt_bwd):
    run_ranks(_worker, 4, causal, striped, opt_bwd, 2, torch.int32,
              what="segment double ring")


def _worker_no_ids(rank, world):
    """Without segment_ids the provider calls carry no seg keyword: a
    provider that predates it (tests/cpu_tile_provider.py) still serves."""
    from burst_attn_amd import burst_attn_func
    from burst_attn_amd.tile import _set_tile_provider_for_testing
    from .cpu_tile_provider import OracleTileProvider

    _set_tile_provider_for_testing(OracleTileProvider())
    g = torch.Generator().manual_seed(rank)
    q, k, v = (torch.randn(1, 32, 2, 32, generator=g, requires_grad=True)
               for _ in range(3))
    o = burst_attn_func(q, k, v, None, "cuda", True, segment_ids=None)
    torch.autograd.grad(o, (q, k, v), torch.ones_like(o))


def test_no_ids_passes_no_seg_keyword():
    run_ranks(_worker_no_ids, 2, what="id-free ring")
