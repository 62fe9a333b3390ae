"""Segment-aware oracle tile provider — TEST INFRASTRUCTURE ONLY.

Lets the product's ring orchestration run on CPU (gloo) with segment ids:
tile calls that carry ``seg=(q_seg, kv_seg)`` compute with the masked
reference of tests/segment_refs.py, calls without it fall through to the
plain oracle provider.  Every ``seg`` handed in is recorded (dtype, shape,
contiguity of the last dim, and the values), so a test can pin what the
ring passes and that, from round 2 on, the travelling side's ids are the
ones that came over the wire.
"""

import torch

import oracle

from . import segment_refs as sr
from .gqa_cpu_provider import GqaOracleTileProvider


class SegOracleTileProvider(GqaOracleTileProvider):
    def __init__(self):
        super().__init__()
        self.fwd_segs = []  # (q_seg, kv_seg) clones, in call order
        self.bwd_segs = []

    @staticmethod
    def _check(seg, q, k):
        q_seg, kv_seg = seg
        for s, rows in ((q_seg, q.shape[1]), (kv_seg, k.shape[1])):
            assert s.dtype == torch.int32, s.dtype
            assert tuple(s.shape) == (q.shape[0], rows), (s.shape, rows)
            assert s.stride(1) == 1 or rows == 1, s.stride()

    def fwd_accum(self, state, q, k, v, scale, causal, row_offset=0,
                  seg=None):
        if seg is None:
            return super().fwd_accum(state, q, k, v, scale, causal, row_offset)
        self._check(seg, q, k)
        self.fwd_segs.append((seg[0].clone(), seg[1].clone()))
        o_i, lse_i = sr.seg_fwd(q, k, v, scale, causal, *seg)
        if state is None:
            assert row_offset == 0
            return [o_i, lse_i.transpose(-2, -1).unsqueeze(-1).contiguous()]
        o, lse = state
        sl = slice(row_offset, row_offset + q.shape[1])
        o[:, sl], lse[:, sl] = oracle.scale_out_lse(o[:, sl], lse[:, sl], o_i,
                                                    lse_i)
        return state

    def bwd_accum(self, do, q, k, v, delta, lse, scale, causal, deterministic,
                  dq, dk, dv, seg=None):
        if seg is None:
            return super().bwd_accum(do, q, k, v, delta, lse, scale, causal,
                                     deterministic, dq, dk, dv)
        self._check(seg, q, k)
        self.bwd_segs.append((seg[0].clone(), seg[1].clone()))
        dq_i, dk_i, dv_i = sr.seg_bwd(do, q, k, v, lse, scale, causal, *seg,
                                      delta=delta)
        dq += dq_i
        dk += dk_i
        dv += dv_i
