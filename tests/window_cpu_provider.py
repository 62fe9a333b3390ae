"""Band-aware oracle tile provider — TEST INFRASTRUCTURE ONLY.

Lets the product's ring orchestration run on CPU (gloo) with a sliding
window: tile calls that carry ``band=(lo, hi)`` compute with the dense
masked reference of tests/segment_refs.py under tests/window_refs.band_mask
(``causal=True`` cuts the band at the diagonal, as the launcher does), calls
without it with the plain GQA oracle provider.  ``fwd_empty_state`` is the
state of "no key seen yet" (o = 0, lse = -inf); the merge tolerates -inf on
either side, where ``oracle.scale_out_lse`` gives NaN.  Every band handed in
is recorded with the shapes it came with.
"""

import torch

from . import segment_refs as sr
from . import window_refs as wr
from .gqa_cpu_provider import GqaOracleTileProvider


def merge_with_inf(o, lse, o_i, lse_i):
    """The LSE merge of (o, lse [B,S,N,1]) with a tile's (o_i, lse_i
    [B,N,S]) in fp64; a side at -inf weighs exactly 0."""
    lse_i = lse_i.transpose(-2, -1).unsqueeze(-1).double()
    lse = lse.double()
    new = torch.logaddexp(lse, lse_i)
    safe = torch.where(new.isinf(), torch.zeros_like(new), new)
    w, w_i = torch.exp(lse - safe), torch.exp(lse_i - safe)
    w = torch.where(lse.isinf(), torch.zeros_like(w), w)
    w_i = torch.where(lse_i.isinf(), torch.zeros_like(w_i), w_i)
    return (w * o.double() + w_i * o_i.double()).float(), new.float()


class WindowOracleTileProvider(GqaOracleTileProvider):
    def __init__(self):
        super().__init__()
        self.fwd_bands = []  # (band or None, causal, Sq, Sk, row_offset)
        self.bwd_bands = []  # (band or None, causal, Sq, Sk)
        self.empty_states = 0

    @staticmethod
    def _mask(q, k, causal, band):
        lo, hi = band
        assert isinstance(lo, int) and isinstance(hi, int) and lo <= hi, band
        if causal:
            assert q.shape[1] == k.shape[1]
            lo = max(lo, 0)
        return wr.band_mask(q.shape[0], q.shape[1], k.shape[1], lo, hi)

    def fwd_empty_state(self, q):
        self.empty_states += 1
        b, s, n, d = q.shape
        return [torch.zeros(b, s, n, d),
                torch.full((b, s, n, 1), float("-inf"))]

    def fwd_accum(self, state, q, k, v, scale, causal, row_offset=0,
                  band=None):
        self.fwd_bands.append((band, causal, q.shape[1], k.shape[1],
                               row_offset))
        if band is None and not (state is not None and
                                 state[1].isinf().any()):
            return super().fwd_accum(state, q, k, v, scale, causal, row_offset)
        if band is None:
            band = (0 if causal else -k.shape[1], q.shape[1])
        o_i, lse_i = sr.seg_fwd(q, k, v, scale, False, None, None,
                                mask=self._mask(q, k, causal, band))
        assert state is not None, "a band call merges into a state"
        o, lse = state
        sl = slice(row_offset, row_offset + q.shape[1])
        o[:, sl], lse[:, sl] = merge_with_inf(o[:, sl], lse[:, sl], o_i, lse_i)
        return state

    def bwd_accum(self, do, q, k, v, delta, lse, scale, causal, deterministic,
                  dq, dk, dv, band=None):
        self.bwd_bands.append((band, causal, q.shape[1], k.shape[1]))
        if band is None:
            return super().bwd_accum(do, q, k, v, delta, lse, scale, causal,
                                     deterministic, dq, dk, dv)
        dq_i, dk_i, dv_i = sr.seg_bwd(do, q, k, v, lse, scale, False, None,
                                      None, delta=delta,
                                      mask=self._mask(q, k, causal, band))
        dq += dq_i
        dk += dk_i
        dv += dv_i
