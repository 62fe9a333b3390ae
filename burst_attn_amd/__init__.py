"""MI355X-native BurstAttention.

A from-scratch gfx950 (CDNA4) implementation of the reference
MayDomine/Burst-Attention hot path: ring-distributed exact attention with
hand-written HIP flash-tile kernels and RCCL P2P over xGMI.

Public API (drop-in for the reference ``burst_attn`` package):
    burst_attn_func, burst_attn_func_striped
Beyond the reference: packed sequences (``segment_ids=``), with the helpers
    segment_ids_from_cu_seqlens, local_segment_ids
"""

from .interface import (  # noqa: F401
    burst_attn_func,
    burst_attn_func_striped,
    OpBurstAttn,
    OpBurstAttnStrip,
)
from .segments import (  # noqa: F401
    local_segment_ids,
    segment_ids_from_cu_seqlens,
)

__version__ = "0.1.0"
