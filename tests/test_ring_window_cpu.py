"""Sliding windows through the ring orchestration on CPU (gloo).

Same structure as tests/test_ring_segments_cpu.py with the band-aware oracle
provider (tests/window_cpu_provider.py) injected: every rank builds the same
full sequence, the reference is the dense masked softmax on it under
``global_window_mask``, and each rank compares its chunk.  Also pins what
the ring hands the provider (bands as Python ints, a state that starts
empty, nothing computed in a round without a visible pair) and the argument
validation.
"""

import numpy as np
import pytest
import torch
import torch.distributed as dist

from oracle.partition import get_chunk

from .gloo_ranks import run_ranks
from .test_ring_cpu import ATOL, RTOL

B, S_LOCAL, N, NK, D = 2, 12, 4, 2, 16

# (window, causal): one narrower than a zigzag half, an unbounded-left one
# under causal written without the flag, a two-sided one, and one that leaves
# whole rounds without a visible pair at W = 3 and 4
WINDOWS = [((5, 0), True), ((-1, 0), False), ((4, 3), False),
           ((30, 0), True), ((3, 0), True)]


def _worker(rank, world, window, causal, striped, opt_bwd, local):
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped
    from burst_attn_amd.interface import (_window_layout, get_partition_id,
                                          window_tiles)
    from burst_attn_amd.tile import _set_tile_provider_for_testing
    from . import segment_refs as sr
    from . import window_refs as wr
    from .window_cpu_provider import WindowOracleTileProvider

    P = WindowOracleTileProvider()
    _set_tile_provider_for_testing(P)
    double_group = [None, None]
    if local:
        ranks = np.arange(world).reshape(-1, local)
        intra = [dist.new_group(list(r)) for r in ranks]
        inter = [dist.new_group(list(r)) for r in ranks.T]
        double_group = [intra[rank // local], inter[rank % local]]

    s = S_LOCAL * world
    g = torch.Generator().manual_seed(4242 + world)
    q = torch.randn(B, s, N, D, generator=g)
    k = torch.randn(B, s, NK, D, generator=g)
    v = torch.randn(B, s, NK, D, generator=g)
    do = torch.randn(B, s, N, D, generator=g)
    sc = 1.0 / D ** 0.5
    mask = wr.global_window_mask(s, *window, causal).expand(B, -1, -1)
    o_ref, lse_ref = sr.seg_fwd(q, k, v, sc, False, None, None, mask=mask)
    dq_ref, dk_ref, dv_ref = sr.seg_bwd(do, q, k, v, lse_ref, sc, False, None,
                                        None, o=o_ref, mask=mask)

    zig = causal and not striped
    ch = lambda t: get_chunk(t, 1, rank, world, zigzag=zig, striped=striped)
    qc, kc, vc = (ch(t).requires_grad_() for t in (q, k, v))
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(qc, kc, vc, None, "cuda", causal, opt_bwd, False, None,
             double_group, window_size=window)
    dq, dk, dv = torch.autograd.grad(o, (qc, kc, vc), ch(do))
    torch.testing.assert_close(o, ch(o_ref), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(dv, ch(dv_ref), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(dk, ch(dk_ref), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(dq, ch(dq_ref), rtol=RTOL, atol=ATOL)

    # what the provider saw: one empty state, then exactly the sub-tiles of
    # window_tiles, round by round, bands as Python ints
    layout = _window_layout("striped" if striped else "zigzag", causal)
    assert P.empty_states == 1
    want_f, want_b = [], []
    for r in range(1, world + 1):
        src = get_partition_id(double_group, r, None)
        for qr, kr, band, tc in window_tiles(layout, rank, src, world, S_LOCAL,
                                             causal, window):
            want_f.append((band, tc, qr.stop - qr.start, kr.stop - kr.start,
                           qr.start))
        for qr, kr, band, tc in window_tiles(layout, src, rank, world, S_LOCAL,
                                             causal, window):
            want_b.append((band, tc, qr.stop - qr.start, kr.stop - kr.start))
    assert P.fwd_bands == want_f
    assert P.bwd_bands == want_b
    for band, *_ in P.fwd_bands + P.bwd_bands:
        assert band is None or all(type(x) is int for x in band)


@pytest.mark.parametrize("opt_bwd", [False, True])
@pytest.mark.parametrize("striped", [False, True])
@pytest.mark.parametrize("window,causal", WINDOWS[:4],
                         ids=lambda x: str(x).replace(" ", ""))
@pytest.mark.parametrize("world", [2, 3])
def test_window_ring_matches_masked_attention(world, window, causal, striped,
                                              opt_bwd):
    run_ranks(_worker, world, window, causal, striped, opt_bwd, 0,
              what="window ring")


@pytest.mark.parametrize("opt_bwd", [False, True])
@pytest.mark.parametrize("striped", [False, True])
@pytest.mark.parametrize("window,causal", [WINDOWS[0], WINDOWS[2], WINDOWS[4]],
                         ids=lambda x: str(x).replace(" ", ""))
def test_window_double_ring(window, causal, striped, opt_bwd):
    run_ranks(_worker, 4, window, causal, striped, opt_bwd, 2,
              what="window double ring")


def test_a_round_without_a_visible_pair_computes_nothing():
    """(3, 0) causal at W = 4, zigzag, s_local = 12: rank 1 holds global
    rows 6..11 and 36..41, rank 3 rows 18..29; no row of rank 1 sees a key of
    rank 3, so that round has no sub-tile."""
    from burst_attn_amd.interface import window_tiles

    assert window_tiles("zigzag", 1, 3, 4, S_LOCAL, True, (3, 0)) == []
    calls = sum(len(window_tiles("zigzag", 1, b, 4, S_LOCAL, True, (3, 0)))
                for b in range(4))
    assert 0 < calls < 4 * 4


@pytest.mark.parametrize("striped", [False, True])
def test_bad_window_raises_before_any_work(striped):
    """Validation needs no process group: it runs before the op."""
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    func = burst_attn_func_striped if striped else burst_attn_func
    q = torch.randn(1, 8, 2, 16)
    ids = torch.zeros(1, 8, dtype=torch.int32)
    for bad in ((1,), (1, 2, 3), (1.0, 0), ("1", 0), (-2, 0), (0, -2), 5,
                (True, 0), [None, 1]):
        with pytest.raises(ValueError, match="window_size"):
            func(q, q, q, window_size=bad)
    with pytest.raises(ValueError,
                       match="window_size.*segment_ids.*not supported "
                             "together yet"):
        func(q, q, q, None, "cuda", True, window_size=(4, 0), segment_ids=ids)
