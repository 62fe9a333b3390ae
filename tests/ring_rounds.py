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
runs; likewise ``SET_CASES`` of tests/test_gpu_ring_sets.py (the head_dim
256, 192 / 128 and fp8 kernel sets; ``replay_ring_fp8`` is their
forward-only replay) and its proof tests/test_ring_sets_cpu.py.
"""

import functools
import math
from collections import namedtuple

import torch

from burst_attn_amd.interface import _dk_tiles, tile_window
from oracle.partition import get_chunk

from . import boundary_inputs as bi

__all__ = ["replay_ring", "replay_ring_fp8", "global_rows", "assemble",
           "allow_mask", "RingCase", "CASES", "SET_CASES", "S_LOCAL",
           "S_LOCAL_TILES", "make_inputs", "make_fp8_inputs", "case_id",
           "scale_of", "FP8", "FP8_NEEDLE_SPAN", "SetCase", "set_case_id",
           "fp8_needle"]


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


def assemble(chunks, layout, dim):
    """The full-sequence tensor of W per-rank chunks."""
    W, s_local = len(chunks), chunks[0].shape[dim]
    shape = list(chunks[0].shape)
    shape[dim] = W * s_local
    full = chunks[0].new_empty(shape)
    for r, c in enumerate(chunks):
        full.index_copy_(dim, global_rows(layout, r, W, s_local)
                         .to(c.device), c)
    return full


_assemble = assemble  # the name the segment and window replays import


def replay_ring(P, q, k, v, do, W, scale, causal, layout,
                deterministic=False):
    """(o, lse, dq, dk, dv) of the full sequence: o in q's dtype [B,S,N,Dv],
    lse fp32 [B,N,S], dq fp32 [B,S,N,D], dk fp32 [B,S,Nk,D], dv fp32
    [B,S,Nk,Dv]; Dv is v's width, which may differ from D.  P is any
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
    dvs = [torch.zeros(t.shape, dtype=torch.float32, device=t.device)
           for t in vs]
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

    return (assemble(os_, layout, 1), assemble(lses, layout, 2),
            assemble(dqs, layout, 1), assemble(dks, layout, 1),
            assemble(dvs, layout, 1))


def replay_ring_fp8(P, q, k, v, W, scale, causal, layout, descale,
                    out_dtype=torch.float16):
    """Forward only, as ``_ring_forward`` runs fp8 inputs: (o in out_dtype
    [B,S,N,D], lse fp32 [B,N,S]) of the full sequence.  ``descale`` is three
    floats (per-tensor scaling, every call carries them) or a list of the W
    ranks' ``(dq [B,N,s_local], dk [B,Nk,ceil(s_local/64)], dv [B,Nk,D])``
    (block scaling): the call of rank a on the kv of rank b then carries
    ``(dq_a[:, :, qw], _dk_tiles(dk_b, kw, s_local, layout), dv_b)``, dq of
    the q window and dk, dv of the source rank's chunk."""
    assert layout in ("zigzag", "striped")
    qs, ks, vs = (_chunks(t, W, layout) for t in (q, k, v))
    s_local = qs[0].shape[1]
    scaled = not isinstance(descale[0], float)
    os_, lses = [], []
    for rank in range(W):
        state = None
        for r in range(1, W + 1):
            src = (rank - (r - 1)) % W
            qw, kw, tc = tile_window(layout, rank, src, causal, s_local)
            ds = descale
            if scaled:
                ds = (descale[rank][0][:, :, qw],
                      _dk_tiles(descale[src][1], kw, s_local, layout),
                      descale[src][2])
            state = P.fwd_accum(state, qs[rank][:, qw], ks[src][:, kw],
                                vs[src][:, kw], scale, tc,
                                row_offset=qw.start or 0, descale=ds)
        o, lse = P.fwd_finalize(state, out_dtype)
        os_.append(o)
        lses.append(lse)
    return assemble(os_, layout, 1), assemble(lses, layout, 2)


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
    if isinstance(case, SetCase):
        return set_case_id(case)
    return (f"{case.layout}-W{case.W}-{case.family}-lag{case.lag}-"
            f"n{case.n}k{case.nk}-d{case.d}-"
            f"{'causal' if case.causal else 'full'}")


@functools.lru_cache(maxsize=4)
def make_inputs(case, dtype):
    """Full-sequence (q, k, v, do) of a RingCase on the CPU, seeded by the
    case; generated on the whole sequence, then chunked by the replay, so
    the families' hot keys land on the ring's seams."""
    if isinstance(case, SetCase):
        return _make_16bit(case, dtype)
    S = case.W * case.s_local
    seed = 7171 + 13 * S + 3 * case.n + case.nk + case.d + 101 * case.lag
    if case.family == "seam_weighted":
        return bi.seam_weighted(case.b, S, S, case.n, case.nk, case.d, dtype,
                                seed)
    return bi.diag_needle(case.b, S, case.n, case.nk, case.d, dtype, seed,
                          lag=case.lag)


# ---- the same rings through the other kernel sets: head_dim 256, q/k 192
# with v 128, and fp8 e4m3 (per-tensor and block-scaled), each separate
# code with 128-row workgroups of its own.  330 = 2 x 128 + 74 is ragged
# against those too.

SetCase = namedtuple(
    "SetCase", "kset family layout W b s_local n nk d dv lag causal")

# block-scaled fp8 under the zigzag layout needs whole 64-row k tiles in
# both half-chunks: 384 gives a 192-row half of 3 tiles, so a later half's
# dk entries start at tile 3
S_LOCAL_TILES = 384
_WIDTHS = {"d256": (256, 256), "hd192": (192, 128), "fp8": (128, 128),
           "fp8_scaled": (128, 128)}
FP8 = torch.float8_e4m3fn


def _set_cases():
    out = []
    for kset in ("d256", "hd192"):
        d, dv = _WIDTHS[kset]
        for layout in ("zigzag", "striped"):
            for W in (3, 4):
                for lag in (0, 1):
                    heads = ((4, 2), (2, 2)) if (W, lag) == (4, 0) else (
                        (4, 2),)
                    for n, nk in heads:
                        out.append(SetCase(kset, "diag_needle", layout, W, _B,
                                           S_LOCAL, n, nk, d, dv, lag, True))
            out.append(SetCase(kset, "seam_weighted", layout, 3, _B, S_LOCAL,
                               4, 2, d, dv, 0, False))
    for family in ("fp8_realistic", "fp8_needle"):
        for layout in ("zigzag", "striped"):
            for W in (3, 4):
                for lag in (0, 1):
                    out.append(SetCase("fp8", family, layout, W, _B, S_LOCAL,
                                       4, 2, 128, 128, lag, True))
    for layout, s_local in (("zigzag", S_LOCAL_TILES), ("striped", S_LOCAL)):
        for W in (3, 4):
            out.append(SetCase("fp8_scaled", "fp8_pow2", layout, W, _B,
                               s_local, 4, 2, 128, 128, 0, True))
    return out


SET_CASES = _set_cases()


def _seed(case):
    return (7171 + 13 * case.W * case.s_local + 3 * case.n + case.nk + case.d
            + 101 * case.lag)


def _make_16bit(case, dtype):
    S = case.W * case.s_local
    if case.family == "seam_weighted":
        return bi.seam_weighted(case.b, S, S, case.n, case.nk, case.d, dtype,
                                _seed(case), dv=case.dv,
                                extra=bi.BLOCK_SEAMS)
    q, k, v, do = bi.diag_needle(case.b, S, case.n, case.nk, case.d,
                                 torch.float32, _seed(case), lag=case.lag,
                                 dv=case.dv)
    # the rows of a 128-row block's edge weigh double in the backward, as
    # tests/test_gpu_d256.py has them
    do[:, list(bi.BLOCK_SEAMS)] *= bi.DO_GAIN
    return tuple(t.to(dtype) for t in (q, k, v, do))


# exact-P needle: scores in {+3, 0, -8}, a span of 11 <= 12, so that every
# P = 2^(s - max) times the kernel's P scale of 16 is an e4m3 value
FP8_NEEDLE_SPAN = 11
_NEEDLE_HOT, _NEEDLE_COLD = 3.0, -8.0


def fp8_needle(b, s, n, nk, seed, lag=0, d=128):
    """(q8, k8, v8, descale, scale) whose every exp2-domain score is an
    integer (scale = ln 2, unit descales for q and k), so that P is a power
    of two and fp8 adds no error.  q row i is one-hot at channel i mod d;
    key j holds 0 at channel (j + lag) mod d, +3 at channel
    (j - max(lag, 1)) mod d and -8 elsewhere: row i scores 0 on key i - lag
    (allowed, the hot key of a row with no +3 key in reach) and +3 on key
    i + max(lag, 1) (forbidden, hotter), as diag_needle has them, so the
    pairs that decide a row sit on other ranks' tile seams; both repeat
    every d keys.  v is randn in e4m3 at descale 1/4."""
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(s)
    q = torch.zeros(b, s, n, d)
    q[:, i, :, i % d] = 1.0
    k = torch.full((b, s, nk, d), _NEEDLE_COLD)
    k[:, i, :, (i + lag) % d] = 0.0
    k[:, i, :, (i - max(lag, 1)) % d] = _NEEDLE_HOT
    v = torch.randn(b, s, nk, d, generator=g)
    return (q.to(FP8), k.to(FP8), v.to(FP8), (1.0, 1.0, 0.25),
            math.log(2.0))


def _pow2_scales(case, rank):
    """Power-of-two scales of one rank's chunk that vary by row % 5, tile
    % 3, channel % 4, head, batch and rank (tests/test_gpu_fp8_scaled.py's
    _case)."""
    s, D = case.s_local, case.d
    bh = lambda h: (torch.arange(case.b)[:, None, None]
                    + torch.arange(h)[None, :, None])
    dq = 2.0 ** -((torch.arange(s) + rank) % 5 + bh(case.n)).float()
    dk = 2.0 ** -((torch.arange(-(-s // 64)) + rank) % 3 + bh(case.nk)
                  - 1).float()
    dv = 2.0 ** ((torch.arange(D) + rank) % 4 - bh(case.nk)).float()
    return dq, dk, dv


@functools.lru_cache(maxsize=2)
def make_fp8_inputs(case):
    """(q8, k8, v8, descale, scale, (qd, kd, vd)) of an fp8 SetCase on the
    CPU: the full-sequence e4m3 tensors, the descales as replay_ring_fp8
    takes them, the softmax scale and the dequantised fp64 tensors."""
    S = case.W * case.s_local
    if case.family == "fp8_needle":
        q8, k8, v8, ds, scale = fp8_needle(case.b, S, case.n, case.nk,
                                           _seed(case), case.lag)
    elif case.family == "fp8_realistic":
        q, k, v, _ = bi.diag_needle(case.b, S, case.n, case.nk, case.d,
                                    torch.float32, _seed(case), lag=case.lag)
        ds = tuple(float(t.abs().max()) / 448.0 for t in (q, k, v))
        q8, k8, v8 = ((t / x).to(FP8) for t, x in zip((q, k, v), ds))
        scale = scale_of(case)
    else:
        assert case.family == "fp8_pow2"
        g = torch.Generator().manual_seed(_seed(case))
        q8, k8, v8 = (torch.randn(case.b, S, h, case.d, generator=g).to(FP8)
                      for h in (case.n, case.nk, case.nk))
        ds = [_pow2_scales(case, r) for r in range(case.W)]
        scale = scale_of(case)
    if isinstance(ds, tuple):
        deq = tuple(t.double() * x for t, x in zip((q8, k8, v8), ds))
    else:  # each rank's chunk by its own scales
        def spread(rank):
            dq, dk, dv = (t.double() for t in ds[rank])
            return (dq.transpose(1, 2)[..., None],
                    dk.repeat_interleave(64, 2)[:, :, :case.s_local]
                    .transpose(1, 2)[..., None], dv[:, None])
        deq = tuple(
            assemble([c.double() * spread(r)[i] for r, c in enumerate(
                _chunks(t, case.W, case.layout))], case.layout, 1)
            for i, t in enumerate((q8, k8, v8)))
    return q8, k8, v8, ds, scale, deq


def set_case_id(case):
    return (f"{case.kset}-{case.layout}-W{case.W}-{case.family}-"
            f"lag{case.lag}-n{case.n}k{case.nk}-s{case.s_local}-"
            f"{'causal' if case.causal else 'full'}")
