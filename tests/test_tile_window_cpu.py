"""The per-round tile window of the ring (interface.tile_window) against
the sequence partitioning itself: for every pair of ranks, the window's
rows and causal flag must mark exactly the (q token, kv token) pairs that
global causality allows.  No process group, no tensors on the wire."""

import pytest
import torch

from burst_attn_amd.interface import tile_window
from oracle.partition import get_chunk


def _window_mask(window, s_local):
    q_rows, kv_rows, tile_causal = window
    tile = torch.ones(s_local, s_local)[q_rows, kv_rows]
    if tile_causal:
        tile = tile.tril()  # j' <= i' in tile-local coordinates
    mask = torch.zeros(s_local, s_local)
    mask[q_rows, kv_rows] = tile
    return mask.bool()


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("layout,s_local", [("zigzag", 4), ("striped", 3)])
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_window_matches_partition(world, layout, s_local, causal):
    tokens = torch.arange(s_local * world)
    chunk = lambda rank: get_chunk(
        tokens, 0, rank, world,
        zigzag=causal and layout == "zigzag", striped=layout == "striped")
    for a in range(world):
        for b in range(world):
            idx_q, idx_kv = chunk(a), chunk(b)
            want = (idx_kv[None, :] <= idx_q[:, None]) if causal else \
                torch.ones(s_local, s_local, dtype=torch.bool)
            got = _window_mask(tile_window(layout, a, b, causal, s_local), s_local)
            assert torch.equal(got, want), (a, b, got, want)


def test_zigzag_causal_needs_even_length():
    with pytest.raises(AssertionError, match="even per-rank seqlen"):
        tile_window("zigzag", 0, 0, True, 3)
    tile_window("zigzag", 0, 0, False, 3)
    tile_window("striped", 0, 1, True, 3)
