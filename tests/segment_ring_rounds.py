"""Segment-aware lock-step replay of the ring — TEST INFRASTRUCTURE ONLY.

A copy of ``tests/ring_rounds.replay_ring`` that also chunks the
full-sequence ids with the layout and hands every tile call
``seg=(q_ids[:, q_window], kv_ids[:, kv_window])``, exactly as
``burst_attn_amd.interface`` does at W > 1.  ``tile_window`` is the
product's; chunking and reassembly are tests/ring_rounds.py's.
"""

import functools
import math

import torch

from burst_attn_amd.interface import tile_window

from . import segment_refs as sr
from .ring_rounds import S_LOCAL, _assemble, _chunks

B, N, NK = 2, 4, 2


def global_cu(W):
    """Boundaries on a chunk seam (multiples of 165), on 256 and 512, two
    length-1 documents, a document inside one kv tile ([20, 50)) and one
    longer than a rank's 330 rows ([513, 913))."""
    cu = [0, 1, 20, 50, 165, 256, 257, 330, 512, 513, 913]
    if W == 4:
        cu.append(1155)
    return cu + [W * S_LOCAL]


@functools.lru_cache(maxsize=4)
def ring_case(W, d, dtype):
    """Full-sequence inputs, ids and the causal reference, shared by the
    layouts and never modified."""
    S = W * S_LOCAL
    ids = sr.ids_from_cu(global_cu(W), S).expand(B, -1).contiguous()
    q, k, v, do = sr.packed_inputs(B, S, S, N, NK, d, dtype, 5150 + W + d,
                                   ids, True)
    return sr._with_ref(q, k, v, do, ids, ids, True)


def replay_ring_seg(P, q, k, v, do, ids, W, scale, causal, layout,
                    deterministic=False):
    """(o, lse, dq, dk, dv) of the full sequence under segment ids ``ids``
    ([B, S] int32, on q's device)."""
    qs, ks, vs, dos = (_chunks(t, W, layout) for t in (q, k, v, do))
    idc = _chunks(ids, W, layout)
    s_local = qs[0].shape[1]
    os_, lses = [], []
    for rank in range(W):
        state = None
        for r in range(1, W + 1):
            src = (rank - (r - 1)) % W
            qw, kw, tc = tile_window(layout, rank, src, causal, s_local)
            state = P.fwd_accum(state, qs[rank][:, qw], ks[src][:, kw],
                                vs[src][:, kw], scale, tc,
                                row_offset=qw.start or 0,
                                seg=(idc[rank][:, qw], idc[src][:, kw]))
        o, lse = P.fwd_finalize(state, q.dtype)
        os_.append(o)
        lses.append(lse)
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
                        dqs[src][:, qw], dks[rank][:, kw], dvs[rank][:, kw],
                        seg=(idc[src][:, qw], idc[rank][:, kw]))
    return (_assemble(os_, layout, 1), _assemble(lses, layout, 2),
            _assemble(dqs, layout, 1), _assemble(dks, layout, 1),
            _assemble(dvs, layout, 1))


def scale_of(d):
    return 1.0 / math.sqrt(d)
