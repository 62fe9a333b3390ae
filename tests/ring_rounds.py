"""Lock-step replay of the ring on the accumulate API — TEST INFRASTRUCTURE
ONLY.

``replay_ring`` runs W virtual ranks in one process and hands a tile
provider exactly the calls ``burst_attn_amd.interface._ring_forward`` and
``_ring_backward`` make at W > 1: ``fwd_accum`` with carried state on the
windows ``tile_window`` returns (``row_offset`` views, the striped
one-token shift), ``fwd_finalize``, ``bwd_preprocess`` into one reused
buffer, and ``bwd_accum`` into zeroed fp32 accumulators under the
whole-sequence lse and delta.  ``tile_window`` is the product's; the
chunking is ``oracle.partition.get_chunk``; everything else (which rank
meets which in a round, where a chunk's rows sit in the full sequence) is
this module's own.  There is no communication, no wire cast and no
``dq_local`` fold here: those are the driver's and are tested over gloo
(tests/test_ring_cpu.py and its siblings).

tests/ring_sim.py is the stateless counterpart (``fwd`` / ``bwd`` plus a
python merge) with window bookkeeping of its own.

The module also owns the cases of tests/test_gpu_ring_rounds.py and of
the CPU proof tests/test_ring_rounds_cpu.py, so the proof covers what
runs.
"""

import functools
import math
from collections import namedtuple

import torch

from burst_attn_amd.interface import tile_window
from oracle.partition import get_chunk

from . import boundary_inputs as bi

__all__ = ["replay_ring", "global_rows", "allow_mask", "RingCase", "CASES",
           "S_LOCAL", "make_inputs", "case_id", "scale_of"]


def _chunks(t, W, layout, dim=1):
    return [get_chunk(t, dim, r, W, zigzag=layout == "zigzag",
                      striped=layout == "striped") for r in range(W)]


def global_rows(layout, rank, W, s_local):
    """Full-sequence positions of rank's s_local local rows."""
    i = torch.arange(s_local)
    if layout == "striped":
        return i * W + rank
    half = s_local // 2
    return torch.where(i < half, rank * half + i,
                       (2 * W - 1 - rank) * half + (i - half))


def _assemble(chunks, layout, dim):
    W, s_local = len(chunks), chunks[0].shape[dim]
    shape = list(chunks[0].shape)
    shape[dim] = W * s_local
    full = chunks[0].new_empty(shape)
    for r, c in enumerate(chunks):
        full.index_copy_(dim, global_rows(layout, r, W, s_local)
                         .to(c.device), c)
    return full


def replay_ring(P, q, k, v, do, W, scale, causal, layout,
                deterministic=False):
    """(o, lse, dq, dk, dv) of the full sequence: o in q's dtype [B,S,N,D],
    lse fp32 [B,N,S], dq fp32 [B,S,N,D], dk/dv fp32 [B,S,Nk,D].  P is any
    provider with the burst_attn_amd/tile.py contract."""
    assert layout in ("zigzag", "striped")
    qs, ks, vs, dos = (_chunks(t, W, layout) for t in (q, k, v, do))
    s_local = qs[0].shape[1]

    # forward: rank keeps q, round r brings the kv of rank - (r - 1)
    os_, lses = [], []
    for rank in range(W):
        state = None
        for r in range(1, W + 1):
            src = (rank - (r - 1)) % W
            qw, kw, tc = tile_window(layout, rank, src, causal, s_local)
            state = P.fwd_accum(state, qs[rank][:, qw], ks[src][:, kw],
                                vs[src][:, kw], scale, tc,
                                row_offset=qw.start or 0)
        o, lse = P.fwd_finalize(state, q.dtype)
        os_.append(o)
        lses.append(lse)

    # backward: rank keeps k, v, dk, dv; round r brings q, do, o, lse of
    # rank - (r - 1), whose dq collects that tile's contribution
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
            qw, kw, tc = tile_window(layout, src, rank, causal, s_local)
            delta = P.bwd_preprocess(os_[src], dos[src], out=delta_buf)
            P.bwd_accum(dos[src][:, qw], qs[src][:, qw], ks[rank][:, kw],
                        vs[rank][:, kw], delta[:, :, qw],
                        lses[src][:, :, qw], scale, tc, deterministic,
                        dqs[src][:, qw], dks[rank][:, kw], dvs[rank][:, kw])

    return (_assemble(os_, layout, 1), _assemble(lses, layout, 2),
            _assemble(dqs, layout, 1), _assemble(dks, layout, 1),
            _assemble(dvs, layout, 1))


def allow_mask(layout, W, s_local, window=tile_window):
    """The causal [S, S] allow-mask the ring's W x W tiles compose to:
    tile (a, b) allows the pairs of its window, all of them or the lower
    triangle of the window (tile_causal; "strict" leaves the window's
    diagonal out).  With the shipped tile_window this is tril."""
    S = W * s_local
    allow = torch.zeros(S, S, dtype=torch.bool)
    loc = torch.arange(s_local)
    for a in range(W):
        for b in range(W):
            qw, kw, tc = window(layout, a, b, True, s_local)
            qi, kj = loc[qw], loc[kw]
            tile = torch.ones(len(qi), len(kj), dtype=torch.bool)
            if tc:
                assert len(qi) == len(kj)
                tile = tile.tril(-1 if tc == "strict" else 0)
            rows = global_rows(layout, a, W, s_local)[qi]
            cols = global_rows(layout, b, W, s_local)[kj]
            allow[rows[:, None], cols[None, :]] = tile
    return allow


# ---- the cases the GPU tests run and the CPU proof covers

RingCase = namedtuple("RingCase", "family layout W b s_local n nk d lag causal")

# two 256-row workgroups with a 74-row q tail (a multiple of neither 32 nor
# 64), six kv tiles with a ragged last one; the zigzag half, 165 = 128 + 37,
# is odd, so the row_offset m/l views start 660 bytes in; the striped shift
# leaves Sq = Sk = 329
S_LOCAL = 330
_B = 2


def _cases():
    out = []
    for layout in ("zigzag", "striped"):
        for W in (3, 4):
            lags = (0, 1, 2, 3) if (layout, W) == ("striped", 4) else (0, 1)
            for d in (64, 128):
                for n, nk in ((4, 2), (2, 2)):
                    for lag in lags:
                        out.append(RingCase("diag_needle", layout, W, _B,
                                            S_LOCAL, n, nk, d, lag, True))
    for layout in ("zigzag", "striped"):
        for d in (64, 128):
            out.append(RingCase("seam_weighted", layout, 3, _B, S_LOCAL,
                                4, 2, d, 0, False))
    return out


CASES = _cases()


def scale_of(case):
    return 1.0 / math.sqrt(case.d)


def case_id(case):
    return (f"{case.layout}-W{case.W}-{case.family}-lag{case.lag}-"
            f"n{case.n}k{case.nk}-d{case.d}-"
            f"{'causal' if case.causal else 'full'}")


@functools.lru_cache(maxsize=4)
def make_inputs(case, dtype):
    """Full-sequence (q, k, v, do) of a RingCase on the CPU, seeded by the
    case; generated on the whole sequence, then chunked by the replay, so
    the families' hot keys land on the ring's seams."""
    S = case.W * case.s_local
    seed = 7171 + 13 * S + 3 * case.n + case.nk + case.d + 101 * case.lag
    if case.family == "seam_weighted":
        return bi.seam_weighted(case.b, S, S, case.n, case.nk, case.d, dtype,
                                seed)
    return bi.diag_needle(case.b, S, case.n, case.nk, case.d, dtype, seed,
                          lag=case.lag)
