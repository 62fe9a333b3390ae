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

Logit soft-capping: the trailing keyword ``softcap`` (the flash-attn
convention, ``0.0`` = off) replaces every score ``s = q.k * softmax_scale`` by
``softcap * tanh(s / softcap)`` before the softmax, in the forward and the
backward kernels of every round.  The cap is a Python float that every rank
knows: nothing new travels the ring, and each round hands the tile provider
``softcap=`` so that all rounds cap alike and the in-kernel merge holds.
Without a cap the provider calls carry no such keyword.  A cap together with
``segment_ids`` or an effective window is refused.

Block-sparse attention: the trailing keywords ``block_mask`` and
``block_size`` of ``burst_attn_func`` (``torch.bool`` or ``uint8``
``[Bm, Hm, s_local / BS, S_global / BS]``, ``Bm`` 1 or B, ``Hm`` 1 or Nk, BS a
power of two >= 64).  Row ``qb`` is this rank's local query block ``qb`` in
the layout the function already uses (zigzag with ``causal``, contiguous
without), column ``kb`` the GLOBAL key block ``kb``; pair (i, j) is visible
iff its block is set and, with ``causal``, ``j <= i`` on global positions.
The rank's slab stays where q stays: in the forward the origin rank of the
visiting k/v names the slab's columns of each (q piece, kv piece) pair
(``block_tiles``) and the round is one ``fwd_accum(blocks=(sub-view, BS))``
per pair into a state that starts empty; a sub-view without a set block
launches nothing.  In the backward the slab travels with {delta-or-o,
grad_output, q, lse} and the kv-resident rank selects its own columns.  The
sub-views are views: nothing is copied per round.  Without a mask neither the
payloads nor the provider calls change.  A mask together with
``segment_ids``, an effective window, a cap, head_dim 256 or the striped op
is refused.

FP8: with q, k, v of ``torch.float8_e4m3fn`` (head_dim 128) the trailing
keyword ``descale=(sq, sk, sv)`` gives the per-tensor descales (real values
``q8 * sq`` and so on; three positive finite Python floats every rank knows,
default ones).  The call is forward only: o is ``torch.bfloat16``, nothing is
saved, k and v travel the ring as ``uint8`` views of their bytes and every
round hands the tile provider ``descale=``.  Inputs that require grad,
``segment_ids``, an effective window, a cap, a block mask, another head_dim
and a malformed ``descale`` are refused before any round, and so is
``descale`` with 16-bit inputs, whose calls are otherwise unchanged.

Block-scaled FP8: ``descale=(dq, dk, dv)`` may instead be three float32
tensors on q's device, this rank's ``dq [B, N, S_local]`` (per token and head),
``dk [B, Nk, ceil(S_local / 64)]`` (per 64-row tile and KV head) and
``dv [B, Nk, 128]`` (per channel and KV head): what ``quantize_fp8(q, k, v)``
returns for the rank's own shard, with no host sync and nothing all-reduced.
``dq`` stays on the rank; ``dk`` and ``dv`` travel the ring with k and v as
small float32 side payloads; every round hands the tile provider
``descale=(dq[:, :, q_rows], the dk tiles of its k view, dv)``.  A k view must
start on a multiple of 64 rows.  Both layouts' views start at row 0 (the whole
chunk, the first zigzag half, or the striped chunk without its last row); the
causal zigzag op also demands ``S_local % 128 == 0`` so that both half-chunks
are whole tiles, and refuses anything else before any round.  Wrong shapes,
dtypes or devices, a tensor that requires grad and a mix of floats and tensors
are refused as a malformed ``descale`` is.

ALiBi: the trailing keyword ``alibi_slopes`` (the flash-attn convention: an
fp32 tensor ``[N]`` or ``[B, N]`` on q's device, one slope per *query* head)
adds ``-slope[b, h] * |i - j|`` to the score of the query at GLOBAL position i
and the key at global position j, before the softmax and before ``causal``.
The global positions follow the op's data layout as a window's do
(``_window_layout``); ``alibi_tiles`` turns a round into one tile call per (q
piece, kv piece) pair, each with ``alibi=(slopes, offset, stride)`` so that
``stride * (i_local - j_local) + offset`` is the pair's global distance, merged
into a state that starts empty.  The slopes are per head and the same on every
rank: nothing new travels.  They get no gradient, and a tensor that requires
one is refused.  Without slopes neither the provider calls nor the kernels
change.  Slopes together with ``segment_ids``, an effective window, a cap, a
block mask, fp8 inputs, head_dim 256 or the (192, 128) widths are refused.

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
           "OpBurstAttnStrip", "window_tiles", "block_tiles", "alibi_tiles",
           "quantize_fp8"]


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


def block_tiles(a, b, W, s_local, causal):
    """The sub-tiles that one ring round computes of the q chunk owned by
    rank ``a`` against the kv chunk owned by rank ``b`` under a block mask: a
    list of ``(q_rows, kv_rows, kv_global_start, tile_causal)``, one per (q
    piece, kv piece) pair of the two ranks (``_pieces``: two zigzag halves
    each with ``causal``, one contiguous chunk without).  With ``causal`` a
    pair wholly above the diagonal is dropped, the pair on it is a causal
    call and a pair below it a plain one: the decisions of ``tile_window``.
    ``kv_global_start`` locates the kv piece's columns in the mask."""
    layout = "zigzag" if causal else "contiguous"
    out = []
    for lq, nq, Pq, _ in _pieces(layout, a, W, s_local):
        for lk, nk, Pk, _ in _pieces(layout, b, W, s_local):
            if causal and Pk > Pq:
                continue
            out.append((slice(lq, lq + nq), slice(lk, lk + nk), Pk,
                        causal and Pk == Pq))
    return out


def alibi_tiles(layout, a, b, W, s_local, causal):
    """The tile calls that one ring round makes of the q chunk owned by rank
    ``a`` against the kv chunk owned by rank ``b`` with ALiBi: a list of
    ``(q_rows, kv_rows, offset, stride, tile_causal)``, one per (q piece, kv
    piece) pair of the two ranks (``_pieces``) that holds a visible pair.  For
    local rows i of ``q_rows`` and j of ``kv_rows`` (counted from the slices'
    starts) ``stride * (i - j) + offset`` is the distance of their global
    positions.  Which pairs are dropped, causal or plain are the decisions of
    ``tile_window``: unit-stride pieces (zigzag halves, contiguous chunks) are
    aligned and equally long, so with ``causal`` a later kv piece is dropped,
    the same piece is a causal call and an earlier one a plain call; a striped
    pair is the causal tile for ``b <= a`` and the causal tile shifted by one
    row for ``b > a``, whose shift the offset absorbs."""
    out = []
    for lq, nq, Pq, stride in _pieces(layout, a, W, s_local):
        for lk, nk, Pk, _ in _pieces(layout, b, W, s_local):
            q0 = k0 = 0
            tile_causal = False
            if causal and stride == 1:
                if Pk > Pq:
                    continue
                tile_causal = Pk == Pq
            elif causal:
                tile_causal = True
                if Pk > Pq:  # row i sees columns < i: rows 1.., columns ..-1
                    q0, nq, nk = 1, nq - 1, nk - 1
                    if nq < 1:
                        continue
            out.append((slice(lq + q0, lq + q0 + nq),
                        slice(lk + k0, lk + k0 + nk),
                        (Pq + stride * q0) - (Pk + stride * k0), stride,
                        tile_causal))
    return out


def _block_view(slab, bs, q_rows, kv_rows, kv_start):
    """The slab's blocks of local q rows ``q_rows`` against the kv piece
    ``kv_rows`` whose global positions start at ``kv_start``: a view."""
    return slab[:, :, q_rows.start // bs:q_rows.stop // bs,
                kv_start // bs:(kv_start + kv_rows.stop - kv_rows.start) // bs]


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


# (q, k, v) widths of multi-head latent attention heads after the latent
# up-projection: 128 "nope" + 64 rope q/k channels, 128 v/o channels
_MLA_WIDTHS = (192, 192, 128)


def _check_heads(q, k, v):
    """q [B,S,N,H]; k/v [B,S,Nk,H] with N a multiple of Nk (N == Nk is
    plain multi-head attention).  v [B,S,Nk,128] next to H = 192 is the one
    pair of unequal widths with kernels; o then has v's width."""
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
    widths = (q.shape[3], k.shape[3], v.shape[3])
    # one pair of unequal widths has kernels: q/k 192 with v 128 (_MLA_WIDTHS)
    if widths != _MLA_WIDTHS and (widths[1] != widths[0]
                                  or widths[2] != widths[0]):
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


def _check_masks_for_head_dim(q, segment_ids, window):
    """256-wide heads run the plain tile kernels only: refuse the masked
    forms here, before any round, not as a kernel error in mid-ring."""
    if q.shape[3] != 256:
        return
    missing = ("segment_ids" if segment_ids is not None
               else "window_size" if window is not None else None)
    if missing:
        raise ValueError(
            f"head_dim 256 with {missing} is not supported yet: the "
            "segment-id and sliding-window tile kernels exist for head_dim "
            "64 and 128 only"
        )


def _check_masks_for_mla_widths(q, v, segment_ids, window, softcap,
                                block_mask):
    """q/k 192 with v 128 runs the plain tile kernels only: refuse every
    masked form here, before any round."""
    if q.shape[3] == v.shape[3]:
        return
    missing = ("segment_ids" if segment_ids is not None
               else "window_size" if window is not None
               else "softcap" if softcap > 0
               else "block_mask" if block_mask is not None else None)
    if missing:
        raise ValueError(
            f"head_dim {q.shape[3]} (q, k) with {v.shape[3]} (v) with "
            f"{missing} is not supported yet: this shape has the plain tile "
            "kernels only"
        )


def _check_softcap(softcap, segment_ids, window):
    """The cap as a float, 0.0 for "off"."""
    if (isinstance(softcap, bool) or not isinstance(softcap, (int, float))
            or not math.isfinite(softcap) or softcap < 0):
        raise ValueError(
            "softcap must be 0.0 (off) or a positive finite number, got "
            f"{softcap!r}"
        )
    if softcap > 0:
        other = ("segment_ids" if segment_ids is not None
                 else "window_size" if window is not None else None)
        if other:
            raise ValueError(
                f"softcap and {other} are not supported together yet"
            )
    return float(softcap)


def _check_block_mask(block_mask, block_size, q, k, causal, segment_ids,
                      window, softcap):
    """None, or ``(slab, BS)``: this rank's mask as contiguous uint8
    (converted once, here).  Everything that can be said without the world
    size is checked here, before the op; the column count is the op's."""
    if block_mask is None:
        return None
    bs = block_size
    if (isinstance(bs, bool) or not isinstance(bs, int) or bs < 64
            or bs & (bs - 1)):
        raise ValueError(
            f"block_size must be a power of two >= 64, got {bs!r} "
            "(with block_mask)"
        )
    other = ("segment_ids" if segment_ids is not None
             else "window_size" if window is not None
             else "softcap" if softcap > 0 else None)
    if other:
        raise ValueError(
            f"block_mask and {other} are not supported together yet"
        )
    if q.shape[3] == 256:
        raise ValueError(
            "head_dim 256 with block_mask is not supported yet: the "
            "block-sparse tile kernels exist for head_dim 64 and 128 only"
        )
    if not isinstance(block_mask, torch.Tensor):
        raise ValueError(
            f"block_mask must be a tensor, got {type(block_mask).__name__}"
        )
    if block_mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(
            f"block_mask must be torch.bool or uint8, got {block_mask.dtype}"
        )
    if block_mask.device != q.device:
        raise ValueError(
            f"block_mask is on {block_mask.device}, q on {q.device}"
        )
    s_local, unit = q.shape[1], (2 * bs if causal else bs)
    if s_local % unit:
        raise ValueError(
            f"block_mask: the per-rank seqlen {s_local} must be a multiple of "
            f"{'2 * ' if causal else ''}block_size = {unit}"
            + (" (causal: both zigzag pieces start on block boundaries)"
               if causal else "")
        )
    rows = s_local // bs
    shape = tuple(block_mask.shape)
    if (len(shape) != 4 or shape[0] not in (1, q.shape[0])
            or shape[1] not in (1, k.shape[2]) or shape[2] != rows
            or shape[3] < rows or shape[3] % rows):
        raise ValueError(
            "block_mask must be [1 or B, 1 or Nk, s_local / block_size, "
            f"S_global / block_size] = [1|{q.shape[0]}, 1|{k.shape[2]}, "
            f"{rows}, {rows} * world size], got {shape}"
        )
    return block_mask.to(torch.uint8).contiguous(), bs


def _check_alibi(alibi_slopes, q, k, v, segment_ids, window, softcap,
                 block_mask):
    """None, or the slopes as contiguous fp32 ``[1 or B, N]``.  Everything a
    call with slopes cannot have is refused here, before any round."""
    t = alibi_slopes
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise ValueError(
            f"alibi_slopes must be a tensor, got {type(t).__name__}"
        )
    if t.dtype != torch.float32:
        raise ValueError(f"alibi_slopes must be float32, got {t.dtype}")
    B, N = q.shape[0], q.shape[2]
    if tuple(t.shape) not in ((N,), (B, N)):
        raise ValueError(
            f"alibi_slopes must be [N] = [{N}] or [B, N] = [{B}, {N}] (one "
            f"slope per query head), got {tuple(t.shape)}"
        )
    if t.device != q.device:
        raise ValueError(f"alibi_slopes is on {t.device}, q on {q.device}")
    if t.requires_grad:
        raise ValueError(
            "alibi_slopes that require grad are not supported: the slopes "
            "get no gradient"
        )
    other = ("segment_ids" if segment_ids is not None
             else "window_size" if window is not None
             else "softcap" if softcap > 0
             else "block_mask" if block_mask is not None
             else "fp8 inputs" if q.dtype == torch.float8_e4m3fn else None)
    if other:
        raise ValueError(
            f"alibi_slopes and {other} are not supported together yet"
        )
    if q.shape[3] == 256 or q.shape[3] != v.shape[3]:
        raise ValueError(
            f"head_dim {q.shape[3]} (q, k) with {v.shape[3]} (v) with "
            "alibi_slopes is not supported yet: the ALiBi tile kernels exist "
            "for head_dim 64 and 128 only"
        )
    return t.reshape(-1, N).contiguous()


_FP8 = torch.float8_e4m3fn


def _check_fp8(q, k, v, descale, segment_ids, window, softcap, block_mask):
    """None with 16-bit inputs, else the fp8 call's ``(sq, sk, sv)`` floats or
    its ``(dq, dk, dv)`` scale tensors, contiguous.  Everything an fp8 call
    cannot have is refused here, before any round."""
    dtypes = (q.dtype, k.dtype, v.dtype)
    if _FP8 not in dtypes:
        if descale is not None:
            raise ValueError(
                "descale is for fp8 (torch.float8_e4m3fn) q, k, v only, got "
                f"q of {q.dtype}"
            )
        return None
    if dtypes != (_FP8,) * 3:
        raise ValueError(
            f"fp8: q, k and v must all be torch.float8_e4m3fn, got {dtypes}"
        )
    if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
        raise ValueError(
            "fp8 inputs that require grad are not supported: the fp8 kernels "
            "are forward only (there is no fp8 backward)"
        )
    other = ("segment_ids" if segment_ids is not None
             else "window_size" if window is not None
             else "softcap" if softcap > 0
             else "block_mask" if block_mask is not None else None)
    if other:
        raise ValueError(
            f"fp8 with {other} is not supported yet: fp8 inputs have the "
            "plain tile kernels only"
        )
    if (q.shape[3], k.shape[3], v.shape[3]) != (128, 128, 128):
        raise ValueError(
            f"fp8 supports head_dim 128 only, got q {q.shape[3]}, "
            f"k {k.shape[3]}, v {v.shape[3]}"
        )
    if descale is None:
        return (1.0, 1.0, 1.0)
    if (isinstance(descale, (tuple, list)) and len(descale) == 3
            and all(isinstance(x, torch.Tensor) for x in descale)):
        B, S, N, Nk = q.shape[0], q.shape[1], q.shape[2], k.shape[2]
        want = ((B, N, S), (B, Nk, -(-S // 64)), (B, Nk, 128))
        for name, t, shape in zip(("dq", "dk", "dv"), descale, want):
            if (t.dtype != torch.float32 or tuple(t.shape) != shape
                    or t.device != q.device or t.requires_grad):
                raise ValueError(
                    "descale must be (dq, dk, dv) float32 tensors on q's "
                    "device that do not require grad, dq [B, N, S], dk [B, "
                    f"Nk, ceil(S / 64)], dv [B, Nk, 128]: {name} must be "
                    f"{shape}, got {tuple(t.shape)} of {t.dtype} on "
                    f"{t.device}"
                    + (" that requires grad" if t.requires_grad else "")
                )
        return tuple(t.contiguous() for t in descale)
    if (not isinstance(descale, (tuple, list)) or len(descale) != 3
            or any(isinstance(x, bool) or not isinstance(x, (int, float))
                   or not math.isfinite(x) or x <= 0 for x in descale)):
        raise ValueError(
            "descale must be (sq, sk, sv), three positive finite Python "
            "floats, or (dq, dk, dv), three float32 tensors (never a mix), "
            f"got {descale!r}"
        )
    return tuple(float(x) for x in descale)


def _dk_tiles(dk, kv_rows, s_local, layout):
    """The ``dk`` entries of the k view ``kv_rows`` of a rank's ``s_local``
    rows: one per 64-row tile, so the view must start on a tile."""
    start, stop, _ = kv_rows.indices(s_local)
    if start % 64:
        raise ValueError(
            f"descale tensors: the {layout} layout hands the tile kernel a k "
            f"view that starts at row {start}, not a multiple of 64"
        )
    return dk[:, :, start // 64:-(-stop // 64)]


def quantize_fp8(q, k, v):
    """fp16 / bf16 q ``[B, S, N, 128]`` and k, v ``[B, S, Nk, 128]`` ->
    ``(q8, k8, v8, (dq, dk, dv))`` for ``burst_attn_func(..., descale=(dq, dk,
    dv))``: ``torch.float8_e4m3fn`` tensors and their fp32 scales, q per token
    and head, k per 64-row tile and head, v per channel and head of this rank's
    rows.  Three HIP kernels, no host sync, nothing all-reduced: every rank
    quantises its own shard and ``dk``, ``dv`` travel the ring with k and v."""
    P = get_tile_provider()
    (q8, dq), (k8, dk), (v8, dv) = (
        P.quantize_fp8(t, mode)
        for t, mode in ((q, "row"), (k, "tile"), (v, "channel")))
    return q8, k8, v8, (dq, dk, dv)


def _op_args(ids, window, softcap, blocks=None, descale=None, alibi=None):
    """The trailing arguments of the two ops: the ids always, the window, the
    cap, the block mask, the fp8 descales and the ALiBi slopes only when given,
    so that a call without them applies the op with the argument list it had
    before they existed."""
    if alibi is not None:  # never with any of the others
        return (None, None, 0.0, None, 64, None, alibi)
    if descale is not None:  # never with ids, a window, a cap or a mask
        return (None, None, 0.0, None, 64, descale)
    if blocks is not None:
        return (ids, None, 0.0, *blocks)  # never with ids, a window or a cap
    if softcap > 0:
        return (ids, None, softcap)  # never with a window
    return (ids,) if window is None else (ids, window)


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
    softcap: float = 0.0,
    block_mask: torch.Tensor = None,
    block_size: int = 64,
    descale=None,
    alibi_slopes: torch.Tensor = None,
):
    _check_heads(q, k, v)
    window = _check_window(window_size, causal, segment_ids)
    _check_masks_for_head_dim(q, segment_ids, window)
    softcap = _check_softcap(softcap, segment_ids, window)
    _check_masks_for_mla_widths(q, v, segment_ids, window, softcap, block_mask)
    descale = _check_fp8(q, k, v, descale, segment_ids, window, softcap,
                         block_mask)
    blocks = _check_block_mask(block_mask, block_size, q, k, causal,
                               segment_ids, window, softcap)
    alibi = _check_alibi(alibi_slopes, q, k, v, segment_ids, window, softcap,
                         block_mask)
    return OpBurstAttn.apply(
        q, k, v, softmax_scale, flash, causal, optimize_bwd_comm,
        deterministic, process_group, double_group,
        *_op_args(_check_segment_ids(segment_ids, q), window, softcap, blocks,
                  descale, alibi),
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
    softcap: float = 0.0,
    block_mask: torch.Tensor = None,
    block_size: int = 64,
    descale=None,
    alibi_slopes: torch.Tensor = None,
):
    _check_heads(q, k, v)
    if block_mask is not None:
        raise ValueError(
            "burst_attn_func_striped does not support block_mask / "
            "block_size: a global key block is not a run of local rows in "
            "the striped layout; use burst_attn_func"
        )
    window = _check_window(window_size, causal, segment_ids)
    _check_masks_for_head_dim(q, segment_ids, window)
    softcap = _check_softcap(softcap, segment_ids, window)
    _check_masks_for_mla_widths(q, v, segment_ids, window, softcap, None)
    descale = _check_fp8(q, k, v, descale, segment_ids, window, softcap, None)
    alibi = _check_alibi(alibi_slopes, q, k, v, segment_ids, window, softcap,
                         None)
    return OpBurstAttnStrip.apply(
        q, k, v, softmax_scale, flash, causal, optimize_bwd_comm,
        deterministic, process_group, double_group,
        *_op_args(_check_segment_ids(segment_ids, q), window, softcap,
                  descale=descale, alibi=alibi),
    )


def _ring_forward(layout, ctx, q, k, v, softmax_scale=None, flash="cuda",
                  causal=False, optimize_bwd_comm=False, deterministic=False,
                  process_group=None, double_group=[None, None],
                  segment_ids=None, window=None, softcap=0.0, block_mask=None,
                  block_size=64, descale=None, alibi=None):
    """Forward of both layouts: q stays, {k, v} travel the ring (with the
    kv ids, when there are segment ids).  With a window every round is the
    sub-tiles of ``window_tiles``, merged into a state that starts empty; with
    a block mask those of ``block_tiles``, each on its view of the rank's slab.
    With a cap every round's tile call carries it.  With fp8 inputs (``descale``
    given) k and v travel as uint8 views of their bytes, every round's tile
    call carries the descales, o is bf16 and nothing is saved.  With ALiBi
    slopes every round is the tile calls of ``alibi_tiles``, each with the
    position offset and stride of its piece pair, into a state that starts
    empty."""
    _check_flash_arg(flash)
    ctx.alibi = alibi
    ctx.segment_ids = ids = segment_ids
    ctx.blocks = None if block_mask is None else (block_mask, block_size)
    ctx.window = window
    ctx.softcap = softcap
    cap = {"softcap": softcap} if softcap > 0 else {}
    scales = None  # (dq, dk, dv) of a block-scaled fp8 call
    if descale is not None:
        cap = {"descale": descale}  # never together with a softcap
        # the wire carries bytes: RCCL and gloo need no fp8 support
        k, v = k.view(torch.uint8), v.view(torch.uint8)
        if isinstance(descale[0], torch.Tensor):
            scales, cap = descale, {}
            if layout == "zigzag" and causal and q.shape[1] % 128:
                raise ValueError(
                    "descale tensors: the zigzag layout needs a per-rank "
                    f"seqlen that is a multiple of 128, got {q.shape[1]} "
                    "(dk is one scale per 64 k rows, and both half-chunks "
                    "must be whole tiles)"
                )
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
    if descale is None:
        ori_k, ori_v = replicate(k), replicate(v)
    comm_bufs = [torch.empty_like(k), torch.empty_like(v)]
    kv_ids = None
    if ids is not None:
        kv_ids = replicate(ids)
        comm_bufs.append(torch.empty_like(ids))
    if scales is not None:  # dq stays; dk and dv travel with k and v
        dq_s, dk_s, dv_s = scales
        comm_bufs += [torch.empty_like(dk_s), torch.empty_like(dv_s)]
    state = None  # provider-owned carry-in accumulator (in-kernel merge)
    if window is not None:
        state = P.fwd_empty_state(q)
        wlayout = _window_layout(layout, causal)
    if alibi is not None:
        state = P.fwd_empty_state(q)
        wlayout = _window_layout(layout, causal)
    if block_mask is not None:
        if block_mask.shape[3] != W * block_mask.shape[2]:
            raise ValueError(
                f"block_mask has {block_mask.shape[3]} key block columns, "
                f"the {W} ranks' sequence has {W * block_mask.shape[2]} "
                f"blocks of block_size {block_size}"
            )
        state = P.fwd_empty_state(q)
        # one host copy answers "does this sub-view hold a set block" for
        # every round without a device sync per round
        slab_host = block_mask.cpu()
    record = []
    for r in range(1, W + 1):
        src = get_partition_id(double_group, r, process_group)
        record.append(src)
        if window is None and block_mask is None and alibi is None:
            qw, kw, tile_causal = tile_window(layout, rank, src, causal, q.shape[1])
        payload = [k, v] if ids is None else [k, v, kv_ids]
        if scales is not None:
            payload += [dk_s, dv_s]
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
        elif alibi is not None:
            for qw, kw, off, stride, tile_causal in alibi_tiles(
                    wlayout, rank, src, W, q.shape[1], causal):
                state = P.fwd_accum(
                    state, q[:, qw], k[:, kw], v[:, kw], scale, tile_causal,
                    row_offset=qw.start, alibi=(alibi, off, stride))
        elif block_mask is not None:
            for qw, kw, kv0, tile_causal in block_tiles(
                    rank, src, W, q.shape[1], causal):
                if not _block_view(slab_host, block_size, qw, kw, kv0).any():
                    continue  # no set block: nothing to launch
                state = P.fwd_accum(
                    state, q[:, qw], k[:, kw], v[:, kw], scale, tile_causal,
                    row_offset=qw.start,
                    blocks=(_block_view(block_mask, block_size, qw, kw, kv0),
                            block_size))
        else:
            seg = {} if ids is None else {"seg": (ids[:, qw], kv_ids[:, kw])}
            kt, vt = k[:, kw], v[:, kw]
            if descale is not None:
                kt, vt = kt.view(_FP8), vt.view(_FP8)
            if scales is not None:
                cap = {"descale": (dq_s[:, :, qw],
                                   _dk_tiles(dk_s, kw, k.shape[1], layout),
                                   dv_s)}
            state = P.fwd_accum(state, q[:, qw], kt, vt, scale,
                                tile_causal, row_offset=qw.start or 0, **seg,
                                **cap)
        if r != W:
            recv, comm_bufs = _record_stream(*comm_bufs), payload
            k, v = recv[:2]
            if ids is not None:
                kv_ids = recv[2]
            if scales is not None:
                dk_s, dv_s = recv[2:4]
            ring.wait()
    _logger.info("fwd record of rank %d: %s", get_rank(), record)
    # o in q.dtype, lse [B,N,S] fp32 (reference :250-252 semantics)
    if descale is not None:  # forward only: bf16 o, nothing saved
        return P.fwd_finalize(state, torch.bfloat16)[0]
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
    # the q side's slab of the block mask travels with q; this rank selects
    # its own key-block columns of whichever slab is visiting
    blocks = ctx.blocks
    q_slab = None if blocks is None else replicate(blocks[0])
    window = ctx.window
    alibi = ctx.alibi
    cap = {"softcap": ctx.softcap} if ctx.softcap > 0 else {}
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
    if blocks is not None:
        read_bufs.append(torch.empty_like(q_slab))
    for r in range(1, W + 1):
        src = get_partition_id(double_group, r, group)
        if window is None and blocks is None and alibi is None:
            qw, kw, tile_causal = tile_window(layout, src, rank, causal, q.shape[1])
        payload = [dlt, grad_output, q, lse]
        if ids is not None:
            payload.append(q_ids)
        if blocks is not None:
            payload.append(q_slab)
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
        elif alibi is not None:
            tiles = alibi_tiles(_window_layout(layout, causal), src, rank, W,
                                q.shape[1], causal)
            for qr, kr, off, stride, tile_causal in tiles:
                P.bwd_accum(
                    grad_output[:, qr], q[:, qr], k[:, kr], v[:, kr],
                    delta[:, :, qr], lse[:, :, qr], scale, tile_causal,
                    ctx.deterministic, tgt[:, qr], dk[:, kr], dv[:, kr],
                    alibi=(alibi, off, stride),
                )
            # the dq fold covers the union of the round's q rows
            qw = slice(min((t[0].start for t in tiles), default=0),
                       max((t[0].stop for t in tiles), default=0))
        elif blocks is not None:
            # (a sub-view without a set block is not tested for here: that
            # would sync on the slab that just arrived; its kernels leave on
            # their empty lists)
            for qr, kr, kv0, tile_causal in block_tiles(
                    src, rank, W, q.shape[1], causal):
                P.bwd_accum(
                    grad_output[:, qr], q[:, qr], k[:, kr], v[:, kr],
                    delta[:, :, qr], lse[:, :, qr], scale, tile_causal,
                    ctx.deterministic, tgt[:, qr], dk[:, kr], dv[:, kr],
                    blocks=(_block_view(q_slab, blocks[1], qr, kr, kv0),
                            blocks[1]),
                )
            qw = _ALL
        else:
            P.bwd_accum(
                grad_output[:, qw], q[:, qw], k[:, kw], v[:, kw],
                delta[:, :, qw], lse[:, :, qw], scale, tile_causal,
                ctx.deterministic, tgt[:, qw], dk[:, kw], dv[:, kw],
                **({} if ids is None else {"seg": (q_ids[:, qw], ids[:, kw])}),
                **cap,
            )
        if r != W:
            recv, read_bufs = _record_stream(*read_bufs), payload
            dlt, grad_output, q, lse = recv[:4]
            if ids is not None:
                q_ids = recv[4]
            if blocks is not None:
                q_slab = recv[4]
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
        # one None per trailing argument of _op_args beyond the ids
        *((None,) * 6 if alibi is not None
          else (None,) * 4 if blocks is not None else (None, None) if cap
          else () if window is None else (None,)),
    )


class OpBurstAttn(torch.autograd.Function):
    """Zigzag (default) ring attention; q,k,v: [B, S/W, N, H]."""

    forward = staticmethod(functools.partial(_ring_forward, "zigzag"))
    backward = staticmethod(functools.partial(_ring_backward, "zigzag"))


class OpBurstAttnStrip(torch.autograd.Function):
    """Striped ring attention (token t → rank t mod W); q,k,v [B,S/W,N,H]."""

    forward = staticmethod(functools.partial(_ring_forward, "striped"))
    backward = staticmethod(functools.partial(_ring_backward, "striped"))
