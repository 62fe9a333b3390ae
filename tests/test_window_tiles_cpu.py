"""``burst_attn_amd.interface.window_tiles`` against the global window mask,
by brute force, and the routing of window-free calls.

For every layout, ring size and window of the sweep, the allow-matrices of
the sub-tiles of all (q owner a, kv owner b) pairs, scattered to global
positions, must sum to exactly the 0/1 mask of ``global_window_mask``: no
pair missing and none computed twice.  No emitted sub-tile has a row or a
column without a visible pair, and a sub-tile that is a full rectangle or a
full causal square carries no band (it runs the plain kernels).
"""

import pytest
import torch

from burst_attn_amd.interface import window_tiles

from . import window_refs as wr
from .gloo_ranks import run_ranks


def global_rows(layout, rank, W, s_local):
    i = torch.arange(s_local)
    if layout == "striped":
        return i * W + rank
    if layout == "contiguous":
        return rank * s_local + i
    h = s_local // 2
    return torch.where(i < h, rank * h + i, (2 * W - 1 - rank) * h + (i - h))


def _windows(s_local, S):
    h = s_local // 2
    return [(0, 0), (1, 0), (2, 1), (h - 1, 0), (h, 0), (s_local, 0),
            (3 * s_local, -1), (-1, 0), (-1, 2), (0, -1), (S, S)]


def _allow(nq, nk, band, tile_causal):
    if band is not None:
        assert not tile_causal, "a band tile carries its whole mask"
        return wr.band_mask(1, nq, nk, *band)[0]
    if tile_causal:
        assert nq == nk
        return torch.ones(nq, nk, dtype=torch.bool).tril()
    return torch.ones(nq, nk, dtype=torch.bool)


@pytest.mark.parametrize("s_local", [6, 10])
@pytest.mark.parametrize("W", [1, 2, 3, 4])
@pytest.mark.parametrize("layout,causal", [
    ("zigzag", True), ("contiguous", False), ("striped", True),
    ("striped", False)])
def test_sub_tiles_sum_to_the_global_mask(layout, causal, W, s_local):
    S = W * s_local
    rows = [global_rows(layout, r, W, s_local) for r in range(W)]
    for window in _windows(s_local, S):
        want = wr.global_window_mask(S, *window, causal).to(torch.int32)
        got = torch.zeros(S, S, dtype=torch.int32)
        for a in range(W):
            for b in range(W):
                for qr, kr, band, tc in window_tiles(layout, a, b, W, s_local,
                                                     causal, window):
                    nq, nk = qr.stop - qr.start, kr.stop - kr.start
                    assert 0 <= qr.start < qr.stop <= s_local
                    assert 0 <= kr.start < kr.stop <= s_local
                    m = _allow(nq, nk, band, tc)
                    what = (layout, causal, W, s_local, window, a, b, qr, kr,
                            band)
                    assert m.any(1).all() and m.any(0).all(), what
                    if m.all() or (nq == nk and
                                   torch.equal(m, torch.ones_like(m).tril())):
                        assert band is None, what
                    if band is not None:
                        assert all(isinstance(x, int) for x in band), what
                        assert band[0] <= band[1], what
                    got[rows[a][qr][:, None], rows[b][kr][None, :]] += \
                        m.to(torch.int32)
        assert torch.equal(got, want), (layout, causal, W, s_local, window)


class _Recorder:
    """Records every provider call: method, tensor shapes and bytes, and the
    keywords by name."""

    def __init__(self, inner):
        self._inner, self.calls = inner, []

    def __getattr__(self, name):
        fn = getattr(self._inner, name)

        def wrapped(*args, **kw):
            sig = [name] + [
                (tuple(a.shape), a.dtype, a.detach().contiguous().numpy()
                 .tobytes()) if isinstance(a, torch.Tensor) else repr(a)
                for a in args if not isinstance(a, (list, tuple))]
            self.calls.append((sig, sorted(kw)))
            return fn(*args, **kw)

        return wrapped


def _worker_unbounded(rank, world, striped, causal):
    """(-1, -1) and None make the same provider calls with the same bytes and
    no new keyword, and neither goes through window_tiles."""
    import burst_attn_amd.interface as itf
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped
    from burst_attn_amd.tile import _set_tile_provider_for_testing
    from .gqa_cpu_provider import GqaOracleTileProvider

    def boom(*a, **k):
        raise AssertionError("window_tiles called without a window")

    itf.window_tiles = boom
    func = burst_attn_func_striped if striped else burst_attn_func
    runs = []
    for kw in ({}, {"window_size": None}, {"window_size": (-1, -1)}):
        rec = _Recorder(GqaOracleTileProvider())
        _set_tile_provider_for_testing(rec)
        g = torch.Generator().manual_seed(40 + rank)
        q = torch.randn(1, 12, 4, 16, generator=g, requires_grad=True)
        k = torch.randn(1, 12, 2, 16, generator=g, requires_grad=True)
        v = torch.randn(1, 12, 2, 16, generator=g, requires_grad=True)
        o = func(q, k, v, None, "cuda", causal, **kw)
        grads = torch.autograd.grad(o, (q, k, v), torch.ones_like(o))
        runs.append((rec.calls, [o.detach()] + list(grads)))
    for calls, outs in runs[1:]:
        assert calls == runs[0][0]
        for x, y in zip(outs, runs[0][1]):
            assert torch.equal(x, y)
    for sig, kws in runs[0][0]:
        assert "band" not in kws and "window" not in kws, (sig[0], kws)
    assert not any(sig[0] == "fwd_empty_state" for sig, _ in runs[0][0])


@pytest.mark.parametrize("striped,causal", [(False, True), (False, False),
                                            (True, True)])
def test_unbounded_window_is_the_window_free_path(striped, causal):
    run_ranks(_worker_unbounded, 2, striped, causal, what="unbounded window")
