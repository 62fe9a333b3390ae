"""Segment ids for packed sequences.

A packed sequence holds several documents back to back; token i carries
the id of its document and may attend only tokens with the same id
(``segment_ids`` of ``burst_attn_func`` / ``burst_attn_func_striped``).
These helpers build the per-token ids from flash-attn style cumulative
lengths and cut out the rows a ring rank holds.  Tail padding is one more
document: a ``cu_seqlens`` that ends before ``total_len`` gives the rest one
extra id.

The row maps restate the layouts of the ring (contiguous chunks; zigzag:
rank r holds chunks ``r`` and ``2W-1-r`` of ``2W``; striped: token t on rank
``t mod W``).  In all three, local order is globally increasing, so the
local ids of a packed sequence are non-decreasing, which is what the
kernels' tile skipping is guaranteed for.
"""

import torch

__all__ = ["segment_ids_from_cu_seqlens", "local_segment_ids"]

LAYOUTS = ("contiguous", "zigzag", "striped")


def segment_ids_from_cu_seqlens(cu_seqlens, total_len):
    """int32 ``[total_len]`` ids: token t of document d (``cu_seqlens[d] <=
    t < cu_seqlens[d + 1]``) gets id d; tokens from ``cu_seqlens[-1]`` on
    (padding) get one more id.  ``cu_seqlens`` starts at 0 and does not
    decrease (an empty document just leaves its id unused)."""
    cu = torch.as_tensor(cu_seqlens, dtype=torch.int64).flatten()
    if cu.numel() < 1 or int(cu[0]) != 0:
        raise ValueError("cu_seqlens must start with 0")
    if cu.numel() > 1 and bool((cu[1:] < cu[:-1]).any()):
        raise ValueError("cu_seqlens must not decrease")
    if int(cu[-1]) > total_len:
        raise ValueError(
            f"cu_seqlens ends at {int(cu[-1])}, past total_len={total_len}"
        )
    pos = torch.arange(total_len, dtype=torch.int64, device=cu.device)
    # number of boundaries at or before t, minus one, is t's document
    return (torch.searchsorted(cu[1:].contiguous(), pos, right=True)).to(torch.int32)


def local_segment_ids(ids, layout, rank, world):
    """Rows of ``ids`` (``[..., S]``, sequence last) that ring rank ``rank``
    of ``world`` holds in ``layout``: the same rows, in the same order, as
    that rank's q/k/v."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {LAYOUTS}, got {layout!r}")
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} outside a ring of {world}")
    s = ids.shape[-1]
    parts = 2 * world if layout == "zigzag" else world
    if s % parts != 0:
        raise ValueError(
            f"sequence length {s} is not a multiple of {parts} ({layout}, "
            f"world {world})"
        )
    if layout == "striped":
        return ids[..., rank::world].contiguous()
    if layout == "zigzag":
        c = s // parts
        lo, hi = rank, parts - 1 - rank
        return torch.cat(
            [ids[..., lo * c:(lo + 1) * c], ids[..., hi * c:(hi + 1) * c]], dim=-1
        ).contiguous()
    c = s // world
    return ids[..., rank * c:(rank + 1) * c].contiguous()
