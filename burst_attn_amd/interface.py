"""BurstAttention ring orchestration — public API and autograd layer.

Drop-in for the reference's ``burst_attn/burst_attn_interface.py``:
``burst_attn_func`` / ``burst_attn_func_striped`` keep the exact signature
and torch.autograd semantics (reference ``:135-158`` / ``:109-132``; grads
for q, k, v only, ``:398``).  Layout is the flash layout ``[B, S, N, H]``
(class docstring ``:162-168``); ``process_group`` is a torch.distributed
ProcessGroup (None → WORLD).

MI355X-first redesign decisions (vs the reference):
  * ONE local-tile backend — the gfx950 HIP kernel pair behind
    ``tile.get_tile_provider()`` — instead of the reference's
    cuda/triton/math dispatch (``:40-51``).  The ``flash`` argument is
    accepted for signature compatibility; the math-path layout
    (``flash`` not in {"cuda","triton"}; [B,N,S,D]) is not supported.
  * dq/dk/dv accumulate in fp32 across ring rounds (the reference
    accumulates in the input dtype, fp16) and are cast to the input dtype
    at the end.
  * ring payloads and round structure are otherwise identical —
    forward rings {k, v} (``:214-242``); backward rings
    {delta-or-o, grad_output, q, lse} plus a separate travelling-dq ring
    with one extra final hop (``:291-396``).

Grouped-query attention (GQA/MQA): ``k``/``v`` may carry fewer heads than
``q`` — q ``[B, S, N, H]``, k/v ``[B, S, Nk, H]`` with ``N % Nk == 0``;
query head h attends KV head ``h // (N // Nk)`` (the flash-attn
convention).  K/V travel the ring UNEXPANDED (the forward payload and the
comm buffers shrink N/Nk-fold), and ``k.grad``/``v.grad`` have Nk heads:
the kernels sum each group's query heads in place.

Packed sequences: the trailing keyword ``segment_ids`` (this rank's
``[B, S_local]`` int32/int64 ids, in the layout of its q/k/v rows; see
``segments.py``) restricts every token to keys of its own id, on top of
``causal``.  The kv ids travel with {k, v} in the forward, the q ids with
{delta-or-o, grad_output, q, lse} in the backward, and each round hands the
tile provider ``seg=(q_ids[:, q_rows], kv_ids[:, kv_rows])``.  The ids are
compared for equality only, so they need nothing from ``tile_window`` and
the causal flag of a tile keeps its meaning.  Without ``segment_ids``
neither the payloads nor the provider calls change.

Sliding windows: the trailing keyword ``window_size=(left, right)`` (the
flash-attn convention: the query at GLOBAL position i sees the key at global
position j iff ``i - left <= j <= i + right``, -1 = unbounded, ``causal``
forces ``right = 0``).  The global position of a local row follows from the
op's data layout (zigzag for ``burst_attn_func`` with ``causal``, contiguous
without, striped for ``burst_attn_func_striped``); ``window_tiles`` turns a
round into sub-tiles, each a plain, causal or ``band=(lo, hi)`` call of the
tile provider, and a round with no visible pair computes nothing (its
communication is unchanged).  Without a window neither the provider calls
nor the kernels change.  A window together with ``segment_ids`` is refused.

The two causal load-balancing layouts (see oracle/partition.py) run the
same code: ``OpBurstAttn`` (zigzag: rank r holds global chunks [r] and
[2W-1-r]) and ``OpBurstAttnStrip`` (striped: token t on rank t mod W) only
name their layout to ``_ring_forward`` / ``_ring_backward``.  All a layout
decides is which rows of the two chunks a round computes, and that is
``tile_window``; the travelling dq hops through ``_TravellingDq``.
"""

import functools
import math
import os

import torch
import torch.distributed as dist

from .comm import Ring, get_rank, replicate
from .log_helper import get_logger
from .tile import get_tile_provider

_logger = get_logger(__name__, level="WARN")

__all__ = ["burst_attn_func", "burst_attn_func_striped", "OpBurstAttn",
           "OpBurstAttnStrip", "window_tiles"]


def get_partition_id(double_group, r, process_group=None):
    """Rank that owns the K/V (fwd) or Q (bwd) chunk held at round r.

    Single ring: r-1 hops behind this rank.  Double ring: from the
    intra/inter positions (reference burst_attn_interface.py:20-37).
    """
    if not double_group or double_group[0] is None:
        world = dist.get_world_size(process_group)
        return (dist.get_rank(process_group) - (r - 1)) % world
    intra = dist.get_world_size(double_group[0])
    inter = dist.get_world_size(double_group[1])
    ii = dist.get_rank(double_group[0])
    ir = dist.get_rank(double_group[1])
    return ((ir - (r - 1) // intra) % inter) * intra + (
        (ii - (r - 1) % intra) % intra
    )


_ALL = slice(None)


def tile_window(layout, a, b, causal, s_local):
    """What one ring round computes of the q chunk owned by rank ``a``
    against the kv chunk owned by rank ``b``: ``(q_rows, kv_rows,
    tile_causal)`` — two slices of the ``s_local`` local rows and the
    causal flag of the tile itself.  Forward has a = this rank and b = the
    source of the round's kv; backward a = the source of the round's q and
    b = this rank.  The layouts are those of ``oracle/partition.py``."""
    if layout == "zigzag" and causal:
        assert s_local % 2 == 0, (
            "zigzag causal needs an even per-rank seqlen (the rank holds "
            "two half-chunks)"
        )
    if not causal or a == b:
        return _ALL, _ALL, causal
    if layout == "striped":
        # local token i of rank r is global i*W + r: row i sees columns
        # <= i of an earlier rank's kv, < i of a later rank's — the causal
        # tile shifted by one token (reference :463-475, :557-585)
        return (_ALL, _ALL, True) if b < a else (slice(1, None), slice(None, -1), True)
    # zigzag, rank r holds global chunks [r] and [2W-1-r]: of an earlier
    # rank's kv only chunk [b] is visible, to all of q (:225-231, :347-367);
    # of a later rank's all is visible, to q's second half only (:232-235,
    # :322-345)
    half = s_local // 2
    return (_ALL, slice(None, half), False) if b < a else (slice(half, None), _ALL, False)


# an unbounded side of a band, as a bound the tile provider accepts (the
# launchers clamp far below it)
BAND_INF = 1 << 40


def _pieces(layout, rank, W, s_local):
    """The runs of a rank's local rows that are arithmetic in the global
    position: ``(local_start, rows, global_start, stride)``."""
    if layout == "zigzag":
        assert s_local % 2 == 0, (
            "zigzag needs an even per-rank seqlen (the rank holds two "
            "half-chunks)"
        )
        h = s_local // 2
        return [(0, h, rank * h, 1), (h, h, (2 * W - 1 - rank) * h, 1)]
    if layout == "contiguous":
        return [(0, s_local, rank * s_local, 1)]
    if layout == "striped":
        return [(0, s_local, rank, W)]
    raise ValueError(f"unknown layout {layout!r}")


def window_tiles(layout, a, b, W, s_local, causal, window):
    """The sub-tiles that one ring round computes of the q chunk owned by
    rank ``a`` against the kv chunk owned by rank ``b`` under the window
    ``(left, right)`` on global positions: a list of ``(q_rows, kv_rows,
    band_or_None, tile_causal)``, two slices of the ``s_local`` local rows,
    the band ``(lo, hi)`` on the row indices of those two views (visible iff
    ``lo <= i - j <= hi``) and the causal flag of the tile call.

    Every (q piece, kv piece) pair of the two ranks (``_pieces``) has a band
    in piece-local indices: with global starts Pq, Pk and unit stride,
    ``i - j`` must lie in ``[-R - (Pq - Pk), L - (Pq - Pk)]``; with stride W
    (striped) in ``[ceil((-R - (a - b)) / W), floor((L - (a - b)) / W)]``.
    The pair is trimmed to the rows that see and the keys that are seen, the
    band re-based to the trimmed views, and dropped if nothing is left.  A
    band that covers its whole rectangle becomes a plain call, one that is
    the causal triangle of a square a causal call: both run the kernels a
    ring without a window runs."""
    left, right = window
    L = None if left < 0 else left
    R = 0 if causal else (None if right < 0 else right)
    out = []
    for lq, nq, Pq, stride in _pieces(layout, a, W, s_local):
        for lk, nk, Pk, _ in _pieces(layout, b, W, s_local):
            if stride == 1:
                lo = None if R is None else -R - (Pq - Pk)
                hi = None if L is None else L - (Pq - Pk)
            else:
                lo = None if R is None else -((R + (Pq - Pk)) // stride)
                hi = None if L is None else (L - (Pq - Pk)) // stride
            if lo is not None and hi is not None and lo > hi:
                continue  # striped: no multiple of W inside the window
            # hull: q rows that see a key, keys that are seen
            q0 = 0 if lo is None else max(0, lo)
            q1 = nq - 1 if hi is None else min(nq - 1, hi + nk - 1)
            k0 = 0 if hi is None else max(0, -hi)
            k1 = nk - 1 if lo is None else min(nk - 1, nq - 1 - lo)
            if q0 > q1 or k0 > k1:
                continue
            nq2, nk2 = q1 - q0 + 1, k1 - k0 + 1
            lo2 = -BAND_INF if lo is None else lo - (q0 - k0)
            hi2 = BAND_INF if hi is None else hi - (q0 - k0)
            q_rows = slice(lq + q0, lq + q1 + 1)
            kv_rows = slice(lk + k0, lk + k1 + 1)
            if lo2 <= -(nk2 - 1) and hi2 >= nq2 - 1:
                out.append((q_rows, kv_rows, None, False))
            elif nq2 == nk2 and lo2 == 0 and hi2 >= nq2 - 1:
                out.append((q_rows, kv_rows, None, True))
            else:
                out.append((q_rows, kv_rows, (lo2, hi2), False))
    return out


def _window_layout(layout, causal):
    """The data layout a window's global positions follow: the zigzag op
    holds contiguous chunks when it is not causal."""
    return "contiguous" if layout == "zigzag" and not causal else layout


def _record_stream(*tensors):
    """Stream hygiene for buffers swapped out while RCCL may still read
    them (reference ``burst_utils.py:36-39``)."""
    if torch.cuda.is_available():
        for t in tensors:
            if t.is_cuda:
                t.record_stream(torch.cuda.current_stream())
    return tensors


def _dq_wire_dtype(q, dq_ring):
    """Wire dtype for the travelling dq on the flat ring.

    The reference rings dq in the input dtype (fp16,
    ``burst_attn_interface.py:301,393``); we keep the in-round
    accumulation fp32 and cast at the hop, so the payload matches the
    reference at better numerics.  ``BA_DQ_WIRE=fp32`` restores the fp32
    wire.  The double ring merges/zeros the travelling buffer itself
    (``comm.py:187-218`` semantics), so it keeps the fp32 wire."""
    if dq_ring.world_size <= 1 or dq_ring.double_ring:
        return None
    if os.environ.get("BA_DQ_WIRE", "dtype") == "fp32":
        return None
    return q.dtype


def _check_flash_arg(flash):
    if flash not in ("cuda", "triton"):
        raise ValueError(
            "this MI355X-native BurstAttention has a single HIP tile backend "
            "operating in the flash layout [B,S,N,H]; the reference's math-"
            f"path layout (flash={flash!r}) is not supported"
        )


def _check_heads(q, k, v):
    """q [B,S,N,H]; k/v [B,S,Nk,H] with N a multiple of Nk (N == Nk is
    plain multi-head attention)."""
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError(
            "q, k, v must be [B, S, heads, head_dim]; got shapes "
            f"{tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}"
        )
    N, Nk, Nv = q.shape[2], k.shape[2], v.shape[2]
    if Nk != Nv:
        raise ValueError(
            f"k and v head counts differ: k has Nk={Nk}, v has {Nv} "
            f"(q has N={N})"
        )
    if Nk < 1 or N % Nk != 0:
        raise ValueError(
            f"q heads N={N} must be a multiple of kv heads Nk={Nk} "
            "(grouped-query attention: query head h attends kv head "
            "h // (N // Nk))"
        )
    if k.shape[3] != q.shape[3] or v.shape[3] != q.shape[3]:
        raise ValueError(
            f"head_dim differs: q {q.shape[3]}, k {k.shape[3]}, "
            f"v {v.shape[3]} (N={N}, Nk={Nk})"
        )


def _check_segment_ids(segment_ids, q):
    """None, or this rank's ids as contiguous int32 ``[B, S_local]`` on q's
    device (converted once, here)."""
    if segment_ids is None:
        return None
    if not isinstance(segment_ids, torch.Tensor):
        raise ValueError(
            f"segment_ids must be a tensor, got {type(segment_ids).__name__}"
        )
    if segment_ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(
            f"segment_ids must be int32 or int64, got {segment_ids.dtype}"
        )
    if tuple(segment_ids.shape) != (q.shape[0], q.shape[1]):
        raise ValueError(
            "segment_ids must be [B, S_local] = "
            f"{(q.shape[0], q.shape[1])} like q's rows, got "
            f"{tuple(segment_ids.shape)}"
        )
    if segment_ids.device != q.device:
        raise ValueError(
            f"segment_ids is on {segment_ids.device}, q on {q.device}"
        )
    return segment_ids.to(torch.int32).contiguous()


def _check_window(window_size, causal, segment_ids):
    """None for "no window", else ``(left, right)`` as given."""
    if window_size is None:
        return None
    if (not isinstance(window_size, (tuple, list)) or len(window_size) != 2
            or any(isinstance(x, bool) or not isinstance(x, int)
                   for x in window_size)
            or any(x < -1 for x in window_size)):
        raise ValueError(
            "window_size must be a pair (left, right) of Python ints >= -1 "
            f"(-1 = unbounded), got {window_size!r}"
        )
    left, right = window_size
    if left == -1 and (causal or right == -1):
        return None  # nothing bounded beyond what causal already does
    if segment_ids is not None:
        raise ValueError(
            "window_size and segment_ids are not supported together yet"
        )
    return (left, right)


def burst_attn_func(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    softmax_scale: float = None,
    flash: str = "cuda",
    causal: bool = False,
    optimize_bwd_comm: bool = False,
    deterministic: bool = False,
    process_group=None,
    double_group=[None, None],
    *,
    segment_ids: torch.Tensor = None,
    window_size=None,
):
    _check_heads(q, k, v)
    window = _check_window(window_size, causal, segment_ids)
    return OpBurstAttn.apply(
        q, k, v, softmax_scale, flash, causal, optimize_bwd_comm,
        deterministic, process_group, double_group,
        _check_segment_ids(segment_ids, q),
        *(() if window is None else (window,)),
    )


def burst_attn_func_striped(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    softmax_scale: float = None,
    flash: str = "cuda",
    causal: bool = False,
    optimize_bwd_comm: bool = False,
    deterministic: bool = False,
    process_group=None,
    double_group=[None, None],
    *,
    segment_ids: torch.Tensor = None,
    window_size=None,
):
    _check_heads(q, k, v)
    window = _check_window(window_size, causal, segment_ids)
    return OpBurstAttnStrip.apply(
        q, k, v, softmax_scale, flash, causal, optimize_bwd_comm,
        deterministic, process_group, double_group,
        _check_segment_ids(segment_ids, q),
        *(() if window is None else (window,)),
    )


def _ring_forward(layout, ctx, q, k, v, softmax_scale=None, flash="cuda",
                  causal=False, optimize_bwd_comm=False, deterministic=False,
                  process_group=None, double_group=[None, None],
                  segment_ids=None, window=None):
    """Forward of both layouts: q stays, {k, v} travel the ring (with the
    kv ids, when there are segment ids).  With a window every round is the
    sub-tiles of ``window_tiles``, merged into a state that starts empty."""
    _check_flash_arg(flash)
    ctx.segment_ids = ids = segment_ids
    ctx.window = window
    ctx.dq_group = double_group
    if isinstance(double_group[0], tuple):
        # [(group, dq_group), (group2, dq_group2)] — separate backward dq
        # ring groups (reference :188-194)
        ctx.dq_group = (double_group[0][1], double_group[1][1])
        double_group = (double_group[0][0], double_group[1][0])
    ctx.softmax_scale = scale = (
        1.0 / math.sqrt(q.shape[-1]) if softmax_scale is None else softmax_scale
    )
    ctx.causal = causal
    ctx.optimize_bwd_comm = optimize_bwd_comm
    ctx.deterministic = deterministic
    ctx.process_group = process_group
    ctx.double_group = double_group

    P = get_tile_provider()
    ring = Ring(process_group, double_group)
    W, rank = ring.world_size, ring.rank
    ori_k, ori_v = replicate(k), replicate(v)
    comm_bufs = [torch.empty_like(k), torch.empty_like(v)]
    kv_ids = None
    if ids is not None:
        kv_ids = replicate(ids)
        comm_bufs.append(torch.empty_like(ids))
    state = None  # provider-owned carry-in accumulator (in-kernel merge)
    if window is not None:
        state = P.fwd_empty_state(q)
        wlayout = _window_layout(layout, causal)
    record = []
    for r in range(1, W + 1):
        src = get_partition_id(double_group, r, process_group)
        record.append(src)
        if window is None:
            qw, kw, tile_causal = tile_window(layout, rank, src, causal, q.shape[1])
        payload = [k, v] if ids is None else [k, v, kv_ids]
        if r != W:
            ring.double_ring_send_recv(payload, comm_bufs, r)
            ring.commit()
        if window is not None:
            for qw, kw, band, tile_causal in window_tiles(
                    wlayout, rank, src, W, q.shape[1], causal, window):
                state = P.fwd_accum(
                    state, q[:, qw], k[:, kw], v[:, kw], scale, tile_causal,
                    row_offset=qw.start,
                    **({} if band is None else {"band": band}))
        else:
            seg = {} if ids is None else {"seg": (ids[:, qw], kv_ids[:, kw])}
            state = P.fwd_accum(state, q[:, qw], k[:, kw], v[:, kw], scale,
                                tile_causal, row_offset=qw.start or 0, **seg)
        if r != W:
            recv, comm_bufs = _record_stream(*comm_bufs), payload
            k, v = recv[:2]
            if ids is not None:
                kv_ids = recv[2]
            ring.wait()
    _logger.info("fwd record of rank %d: %s", get_rank(), record)
    # o in q.dtype, lse [B,N,S] fp32 (reference :250-252 semantics)
    out, lse = P.fwd_finalize(state, q.dtype)
    ctx.save_for_backward(q, ori_k, ori_v, lse, replicate(out))
    return out


class _TravellingDq:
    """The hop of the dq that follows its q chunk around ``ring``, in one
    of two forms (``_dq_wire_dtype``): cast into a wire buffer, sent, and
    copied back into the fp32 dq; or the fp32 dq itself sent and swapped
    with the buffer it was received into."""

    def __init__(self, ring, q, dq):
        self.ring = ring
        self.wire_dtype = _dq_wire_dtype(q, ring)
        if self.wire_dtype is not None:
            self.wire_s = torch.empty(q.shape, dtype=self.wire_dtype, device=q.device)
            self.wire_r = torch.empty_like(self.wire_s)
        else:
            # the fp32 swap buffer is only needed on the fp32-wire path
            self.buf = [torch.empty_like(dq)]

    def start(self, dq, r):
        """Queue and commit the hop of round ``r``."""
        if self.wire_dtype is not None:
            self.wire_s.copy_(dq)
            self.ring.send_recv([self.wire_s], [self.wire_r])
        else:
            self.ring.double_ring_send_recv_q([dq], self.buf, r)
        self.ring.commit()

    def finish(self, dq):
        """Wait for the hop; returns the dq that arrived."""
        self.ring.wait()
        if self.wire_dtype is not None:
            dq.copy_(self.wire_r)
            return dq
        recv, self.buf = _record_stream(*self.buf), [dq]
        return recv[0]


def _ring_backward(layout, ctx, grad_output):
    """Backward of both layouts: k, v, dk, dv stay; {delta-or-o,
    grad_output, q, lse} travel one ring and their dq a second one."""
    q, k, v, lse, o = ctx.saved_tensors
    # this rank's ids: the kv side for the whole backward; a copy of them
    # travels with q as the q side
    ids = ctx.segment_ids
    q_ids = None if ids is None else replicate(ids)
    window = ctx.window
    P = get_tile_provider()
    scale, causal = ctx.softmax_scale, ctx.causal
    grad_output = grad_output.contiguous()
    group, double_group = ctx.process_group, ctx.double_group
    ring = Ring(group, double_group)
    dq_ring = Ring(group, ctx.dq_group)
    W, rank = ring.world_size, ring.rank

    dq = torch.zeros(q.shape, dtype=torch.float32, device=q.device)
    dk = torch.zeros(k.shape, dtype=torch.float32, device=k.device)
    dv = torch.zeros(v.shape, dtype=torch.float32, device=v.device)
    # rank-local staging for rounds whose travelling dq is in flight:
    # kernels accumulate here during the hop, ONE add folds it in
    # after the wait (at W=1 the kernels hit dq directly)
    dq_local = torch.zeros_like(dq) if W > 1 else dq

    if ctx.optimize_bwd_comm:
        # ring the tiny fp32 delta instead of o (reference :269-278)
        dlt = P.bwd_preprocess(o, grad_output)  # [B,N,S] fp32
        delta_buf = None
    else:
        dlt = o  # o travels; delta recomputed per round
        delta_buf = torch.empty(
            q.shape[0], q.shape[2], q.shape[1], dtype=torch.float32,
            device=q.device,
        )
    dq_hop = _TravellingDq(dq_ring, q, dq)
    read_bufs = [torch.empty_like(t) for t in (dlt, grad_output, q, lse)]
    if ids is not None:
        read_bufs.append(torch.empty_like(q_ids))
    for r in range(1, W + 1):
        src = get_partition_id(double_group, r, group)
        if window is None:
            qw, kw, tile_causal = tile_window(layout, src, rank, causal, q.shape[1])
        payload = [dlt, grad_output, q, lse]
        if ids is not None:
            payload.append(q_ids)
        if r != W:
            ring.double_ring_send_recv(payload, read_bufs, r)
            ring.commit()
        if r != 1:
            dq_hop.start(dq, r)
        delta = (
            dlt if ctx.optimize_bwd_comm
            else P.bwd_preprocess(dlt, grad_output, out=delta_buf)
        )
        tgt = dq if r == 1 else dq_local
        if window is not None:
            tiles = window_tiles(_window_layout(layout, causal), src, rank, W,
                                 q.shape[1], causal, window)
            for qr, kr, band, tile_causal in tiles:
                P.bwd_accum(
                    grad_output[:, qr], q[:, qr], k[:, kr], v[:, kr],
                    delta[:, :, qr], lse[:, :, qr], scale, tile_causal,
                    ctx.deterministic, tgt[:, qr], dk[:, kr], dv[:, kr],
                    **({} if band is None else {"band": band}),
                )
            # the dq fold below covers the union of the round's q rows (an
            # empty slice when the round computed nothing)
            qw = slice(min((t[0].start for t in tiles), default=0),
                       max((t[0].stop for t in tiles), default=0))
        else:
            P.bwd_accum(
                grad_output[:, qw], q[:, qw], k[:, kw], v[:, kw],
                delta[:, :, qw], lse[:, :, qw], scale, tile_causal,
                ctx.deterministic, tgt[:, qw], dk[:, kw], dv[:, kw],
                **({} if ids is None else {"seg": (q_ids[:, qw], ids[:, kw])}),
            )
        if r != W:
            recv, read_bufs = _record_stream(*read_bufs), payload
            dlt, grad_output, q, lse = recv[:4]
            if ids is not None:
                q_ids = recv[4]
        ring.wait()
        if r != 1:
            dq = dq_hop.finish(dq)
            # fold this round's local contribution into the received dq
            dq[:, qw] += dq_local[:, qw]
            dq_local[:, qw].zero_()
    # one extra hop returns the travelling dq to its owner (:393-396)
    dq_hop.start(dq, W + 1)
    dq = dq_hop.finish(dq)
    return (
        dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype),
        None, None, None, None, None, None, None, None,
        *(() if window is None else (None,)),
    )


class OpBurstAttn(torch.autograd.Function):
    """Zigzag (default) ring attention; q,k,v: [B, S/W, N, H]."""

    forward = staticmethod(functools.partial(_ring_forward, "zigzag"))
    backward = staticmethod(functools.partial(_ring_backward, "zigzag"))


class OpBurstAttnStrip(torch.autograd.Function):
    """Striped ring attention (token t → rank t mod W); q,k,v [B,S/W,N,H]."""

    forward = staticmethod(functools.partial(_ring_forward, "striped"))
    backward = staticmethod(functools.partial(_ring_backward, "striped"))
