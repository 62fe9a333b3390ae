"""Window-aware lock-step replay of the ring — TEST INFRASTRUCTURE ONLY.

A copy of ``tests/ring_rounds.replay_ring`` driven by the product's
``window_tiles``: every rank starts from ``fwd_empty_state`` and makes one
``fwd_accum`` / ``bwd_accum`` per sub-tile of every round, exactly as
``burst_attn_amd.interface`` does with a window at W > 1, on one device.
Chunking and reassembly cover the three layouts (zigzag, contiguous,
striped) by global row index.

The inputs are the edge needles of tests/window_refs.py on the full
sequence (``lo = -right``, ``hi = left``), at rows chosen so that the four
edge keys of a row straddle a chunk seam (a multiple of 165 = S_LOCAL / 2):
the visible edge key is the last row of one chunk and the hidden one the
first row of the next, or the other way round.
"""

import functools

import torch

from burst_attn_amd.interface import window_tiles

from . import window_refs as wr

S_LOCAL = 330
B, N, NK = 1, 4, 2


def global_rows(layout, rank, W, s_local):
    i = torch.arange(s_local)
    if layout == "striped":
        return i * W + rank
    if layout == "contiguous":
        return rank * s_local + i
    h = s_local // 2
    return torch.where(i < h, rank * h + i, (2 * W - 1 - rank) * h + (i - h))


def _chunks(t, W, layout, dim=1):
    s_local = t.shape[dim] // W
    return [t.index_select(dim, global_rows(layout, r, W, s_local)
                           .to(t.device)).contiguous() for r in range(W)]


def _assemble(chunks, layout, dim):
    W, s_local = len(chunks), chunks[0].shape[dim]
    shape = list(chunks[0].shape)
    shape[dim] = W * s_local
    full = chunks[0].new_empty(shape)
    for r, c in enumerate(chunks):
        full.index_copy_(dim, global_rows(layout, r, W, s_local).to(c.device),
                         c)
    return full


def seam_rows(S, lo, hi):
    """Rows whose band edges fall on the seams at multiples of 165."""
    rows = set()
    for s in range(S_LOCAL // 2, S, S_LOCAL // 2):
        rows.update((s + hi, s - 1 + lo))   # keys (s, s-1) and (s-1, s)
    return tuple(sorted(p for p in rows if 0 <= p < S))


@functools.lru_cache(maxsize=4)
def ring_case(W, window, causal, d, dtype):
    """Full-sequence needle inputs and the dense reference under the global
    window mask; shared by the layouts and never modified."""
    S = W * S_LOCAL
    left, right = window
    lo, hi = (0 if causal else -right), left
    q, k, v, do = wr.needle_inputs(B, S, S, N, NK, d, dtype,
                                   77 + W + d + left, lo, hi,
                                   seam_rows(S, lo, hi))
    mask = wr.global_window_mask(S, left, right, causal).expand(B, -1, -1)
    return wr.with_ref(q, k, v, do, mask)


def replay_window_ring(P, q, k, v, do, W, scale, causal, layout, window,
                       deterministic=False):
    """(o, lse, dq, dk, dv) of the full sequence under ``window``."""
    qs, ks, vs, dos = (_chunks(t, W, layout) for t in (q, k, v, do))
    s_local = qs[0].shape[1]
    os_, lses = [], []
    for rank in range(W):
        state = P.fwd_empty_state(qs[rank])
        for r in range(1, W + 1):
            src = (rank - (r - 1)) % W
            for qw, kw, band, tc in window_tiles(layout, rank, src, W,
                                                 s_local, causal, window):
                state = P.fwd_accum(
                    state, qs[rank][:, qw], ks[src][:, kw], vs[src][:, kw],
                    scale, tc, row_offset=qw.start,
                    **({} if band is None else {"band": band}))
        o, lse = P.fwd_finalize(state, q.dtype)
        os_.append(o)
        lses.append(lse)
    dqs = [torch.zeros(t.shape, dtype=torch.float32, device=t.device)
           for t in qs]
    dks = [torch.zeros(t.shape, dtype=torch.float32, device=t.device)
           for t in ks]
    dvs = [torch.zeros_like(t) for t in dks]
    b, _, n, _ = qs[0].shape
    delta_buf = torch.empty(b, n, s_local, dtype=torch.float32,
                            device=q.device)
    for rank in range(W):
        for r in range(1, W + 1):
            src = (rank - (r - 1)) % W
            delta = P.bwd_preprocess(os_[src], dos[src], out=delta_buf)
            for qw, kw, band, tc in window_tiles(layout, src, rank, W,
                                                 s_local, causal, window):
                P.bwd_accum(dos[src][:, qw], qs[src][:, qw], ks[rank][:, kw],
                            vs[rank][:, kw], delta[:, :, qw],
                            lses[src][:, :, qw], scale, tc, deterministic,
                            dqs[src][:, qw], dks[rank][:, kw],
                            dvs[rank][:, kw],
                            **({} if band is None else {"band": band}))
    return (_assemble(os_, layout, 1), _assemble(lses, layout, 2),
            _assemble(dqs, layout, 1), _assemble(dks, layout, 1),
            _assemble(dvs, layout, 1))
