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

__all__ = ["burst_attn_func", "burst_attn_func_striped", "OpBurstAttn", "OpBurstAttnStrip"]


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
):
    _check_heads(q, k, v)
    return OpBurstAttn.apply(
        q, k, v, softmax_scale, flash, causal, optimize_bwd_comm,
        deterministic, process_group, double_group,
        _check_segment_ids(segment_ids, q),
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
):
    _check_heads(q, k, v)
    return OpBurstAttnStrip.apply(
        q, k, v, softmax_scale, flash, causal, optimize_bwd_comm,
        deterministic, process_group, double_group,
        _check_segment_ids(segment_ids, q),
    )


def _ring_forward(layout, ctx, q, k, v, softmax_scale=None, flash="cuda",
                  causal=False, optimize_bwd_comm=False, deterministic=False,
                  process_group=None, double_group=[None, None],
                  segment_ids=None):
    """Forward of both layouts: q stays, {k, v} travel the ring (with the
    kv ids, when there are segment ids)."""
    _check_flash_arg(flash)
    ctx.segment_ids = ids = segment_ids
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
    record = []
    for r in range(1, W + 1):
        src = get_partition_id(double_group, r, process_group)
        record.append(src)
        qw, kw, tile_causal = tile_window(layout, rank, src, causal, q.shape[1])
        payload = [k, v] if ids is None else [k, v, kv_ids]
        if r != W:
            ring.double_ring_send_recv(payload, comm_bufs, r)
            ring.commit()
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
    )


class OpBurstAttn(torch.autograd.Function):
    """Zigzag (default) ring attention; q,k,v: [B, S/W, N, H]."""

    forward = staticmethod(functools.partial(_ring_forward, "zigzag"))
    backward = staticmethod(functools.partial(_ring_backward, "zigzag"))


class OpBurstAttnStrip(torch.autograd.Function):
    """Striped ring attention (token t → rank t mod W); q,k,v [B,S/W,N,H]."""

    forward = staticmethod(functools.partial(_ring_forward, "striped"))
    backward = staticmethod(functools.partial(_ring_backward, "striped"))
