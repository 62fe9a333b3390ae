"""ALiBi without a GPU: the interface's refusals, ``alibi_tiles`` against brute
force on global positions, and the ring on gloo with the fp64 provider of
tests/alibi_cpu_provider.py against whole-sequence fp64 attention with
``-slope * |i - j|`` added to the scores.
"""

import numpy as np
import pytest
import torch
import torch.distributed as dist

from oracle.partition import get_chunk

from .alibi_cpu_provider import (AlibiTileProvider, alibi_attention,
                                 std_slopes)
from .gloo_ranks import run_ranks
from .test_ring_cpu import ATOL, RTOL

B, S_LOCAL, N, NK, D = 2, 12, 4, 2, 16
ONES = torch.ones(2)
TOGETHER = "alibi_slopes and {} are not supported together yet"


@pytest.mark.parametrize("striped", [False, True], ids=["zigzag", "striped"])
@pytest.mark.parametrize("kw,d,match", [
    (dict(alibi_slopes=[0.5, 0.25]), 16, "must be a tensor"),
    (dict(alibi_slopes=ONES.double()), 16, "float32"),
    (dict(alibi_slopes=torch.ones(3)), 16, r"\[N\] = \[2\]"),
    (dict(alibi_slopes=torch.ones(1, 1, 2)), 16, r"\[B, N\]"),
    (dict(alibi_slopes=torch.ones(2, device="meta")), 16, "is on meta"),
    (dict(alibi_slopes=torch.ones(2, requires_grad=True)), 16, "require grad"),
    (dict(alibi_slopes=ONES, segment_ids=torch.zeros(1, 128, dtype=torch.int32)),
     16, TOGETHER.format("segment_ids")),
    (dict(alibi_slopes=ONES, window_size=(4, 0)), 16,
     TOGETHER.format("window_size")),
    (dict(alibi_slopes=ONES, softcap=2.0), 16, TOGETHER.format("softcap")),
    (dict(alibi_slopes=ONES, block_mask=torch.ones(1, 1, 2, 2).bool()), 128,
     TOGETHER.format("block_mask")),
    (dict(alibi_slopes=ONES), "fp8", TOGETHER.format("fp8 inputs")),
    (dict(alibi_slopes=ONES), 256, "head_dim 256.*alibi_slopes"),
    (dict(alibi_slopes=ONES), (192, 128), "head_dim 192.*128.*alibi_slopes"),
], ids=lambda x: x if isinstance(x, str) else None)
def test_bad_alibi_raises_before_any_work(kw, d, match, striped):
    """Validation needs no process group: it runs before the op."""
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    if striped and "block_mask" in kw:
        match = "does not support block_mask"  # the striped op's own refusal
    func = burst_attn_func_striped if striped else burst_attn_func
    dq, dv = d if isinstance(d, tuple) else (128, 128) if d == "fp8" else (d, d)
    q, v = torch.randn(1, 128, 2, dq), torch.randn(1, 128, 2, dv)
    if d == "fp8":
        q = v = q.to(torch.float8_e4m3fn)
    with pytest.raises(ValueError, match=match):
        func(q, q, v, **kw)


def _global_rows(layout, rank, W, s_local):
    from burst_attn_amd.interface import _pieces

    g = [0] * s_local
    for l0, n, p0, stride in _pieces(layout, rank, W, s_local):
        g[l0:l0 + n] = range(p0, p0 + stride * n, stride)
    return g


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("layout", ["zigzag", "contiguous", "striped"])
@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_alibi_tiles_cover_each_allowed_pair_once(W, layout, causal):
    """Every allowed (global i, global j) pair is in exactly one tile, and
    there ``stride * (i_loc - j_loc) + offset == i_glob - j_glob``."""
    from burst_attn_amd.interface import alibi_tiles

    s_local = 6
    for a in range(W):
        for b in range(W):
            gq = _global_rows(layout, a, W, s_local)
            gk = _global_rows(layout, b, W, s_local)
            seen = np.zeros((s_local, s_local), dtype=int)
            tiles = alibi_tiles(layout, a, b, W, s_local, causal)
            for qr, kr, off, stride, tc in tiles:
                assert type(off) is int and type(stride) is int and stride >= 1
                assert not tc or qr.stop - qr.start == kr.stop - kr.start
                for i in range(qr.start, qr.stop):
                    for j in range(kr.start, kr.stop):
                        il, jl = i - qr.start, j - kr.start
                        if tc and jl > il:
                            continue
                        seen[i, j] += 1
                        assert stride * (il - jl) + off == gq[i] - gk[j]
            want = np.array([[int(not causal or gk[j] <= gq[i])
                              for j in range(s_local)] for i in range(s_local)])
            assert (seen == want).all(), (a, b, tiles)
            if layout == "zigzag" and causal:
                assert len(tiles) == (3 if a == b else 2)


def _worker(rank, world, causal, striped, opt_bwd, local):
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped
    from burst_attn_amd.tile import _set_tile_provider_for_testing

    _set_tile_provider_for_testing(AlibiTileProvider())
    double_group = [None, None]
    if local:
        ranks = np.arange(world).reshape(-1, local)
        intra = [dist.new_group(list(r)) for r in ranks]
        inter = [dist.new_group(list(r)) for r in ranks.T]
        double_group = [intra[rank // local], inter[rank % local]]

    s = S_LOCAL * world
    g = torch.Generator().manual_seed(5151 + world)
    q, k, v, do = (torch.randn(B, s, h, D, generator=g, dtype=torch.float64)
                   for h in (N, NK, NK, N))
    slopes = std_slopes(B, N)  # differ per batch row and per query head
    qr, kr, vr = (t.clone().requires_grad_() for t in (q, k, v))
    o_ref, _ = alibi_attention(qr, kr, vr, D ** -0.5, causal, slopes)
    refs = (o_ref, *torch.autograd.grad(o_ref, (qr, kr, vr), do))

    zig = causal and not striped
    ch = lambda t: get_chunk(t, 1, rank, world, zigzag=zig, striped=striped)
    qc, kc, vc = (ch(t).requires_grad_() for t in (q, k, v))
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(qc, kc, vc, None, "cuda", causal, opt_bwd, False, None,
             double_group, alibi_slopes=slopes)
    got = (o, *torch.autograd.grad(o, (qc, kc, vc), ch(do)))
    for name, a, r in zip(("o", "dq", "dk", "dv"), got, refs):
        torch.testing.assert_close(a, ch(r.detach()), rtol=RTOL, atol=ATOL,
                                   msg=lambda m, name=name: f"{name}: {m}")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("striped", [False, True], ids=["zigzag", "striped"])
@pytest.mark.parametrize("world", [2, 3])
def test_alibi_ring_matches_whole_sequence(world, striped, causal):
    """(optimize_bwd_comm at W = 3)"""
    run_ranks(_worker, world, causal, striped, world == 3, 0,
              what="alibi ring")


def test_alibi_double_ring():
    run_ranks(_worker, 4, True, False, False, 2, what="alibi double ring")
