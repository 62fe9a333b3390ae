"""Grouped-query oracle tile provider and helpers — TEST INFRASTRUCTURE ONLY.

The GQA reference for every test is the existing equal-heads oracle on K/V
expanded with ``repeat_interleave(G, dim=2)`` (query head h then sits next
to its own copy of KV head h // G), with dk/dv reduced back over each
group as ``view(B, S, Nk, G, D).sum(3)`` in fp32.

``GqaOracleTileProvider`` applies that wrapper to the tile calls, so the
product's ring orchestration can run on CPU with Nk-head K/V.  It also
records the head count of every K/V it is handed, which lets a test pin
that K/V travel the ring unexpanded.
"""

import torch

import oracle

from .cpu_tile_provider import OracleTileProvider


def expand_kv(t, n_q):
    """[B, S, Nk, D] -> [B, S, N, D]: each KV head repeated G = N / Nk times."""
    nk = t.shape[2]
    assert n_q % nk == 0, (n_q, nk)
    return t.repeat_interleave(n_q // nk, dim=2)


def reduce_kv_grad(g, nk):
    """[B, S, N, D] fp32 -> [B, S, Nk, D]: sum over each group's G heads."""
    b, s, n, d = g.shape
    return g.to(torch.float32).reshape(b, s, nk, n // nk, d).sum(3)


def gqa_full_reference(q, k, v, do, scale, causal):
    """Full-sequence (o, dq, dk, dv) for Nk-head k/v via the expanded oracle."""
    n, nk = q.shape[2], k.shape[2]
    o, dq, dk, dv = oracle.ring_forward_backward_reference(
        q, expand_kv(k, n), expand_kv(v, n), do, scale, causal
    )
    return o, dq, reduce_kv_grad(dk, nk), reduce_kv_grad(dv, nk)


class GqaOracleTileProvider(OracleTileProvider):
    def __init__(self):
        # (k heads, v heads) of every tile call, in call order
        self.fwd_kv_heads = []
        self.bwd_kv_heads = []

    def fwd(self, q, k, v, scale, causal):
        n = q.shape[2]
        return super().fwd(q, expand_kv(k, n), expand_kv(v, n), scale, causal)

    def bwd(self, do, q, k, v, delta, lse, scale, causal, deterministic):
        n, nk = q.shape[2], k.shape[2]
        dq, dk, dv = super().bwd(do, q, expand_kv(k, n), expand_kv(v, n),
                                 delta, lse, scale, causal, deterministic)
        return dq, reduce_kv_grad(dk, nk), reduce_kv_grad(dv, nk)

    def bwd_accum(self, do, q, k, v, delta, lse, scale, causal, deterministic,
                  dq, dk, dv):
        self.bwd_kv_heads.append((k.shape[2], v.shape[2]))
        assert dk.shape == k.shape and dv.shape == v.shape, (dk.shape, k.shape)
        dq_i, dk_i, dv_i = self.bwd(do, q, k, v, delta, lse, scale, causal,
                                    deterministic)
        dq += dq_i
        dk += dk_i
        dv += dv_i

    def fwd_accum(self, state, q, k, v, scale, causal, row_offset=0):
        self.fwd_kv_heads.append((k.shape[2], v.shape[2]))
        n = q.shape[2]
        return super().fwd_accum(state, q, expand_kv(k, n), expand_kv(v, n),
                                 scale, causal, row_offset)
