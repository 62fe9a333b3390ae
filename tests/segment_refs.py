"""Reference, inputs and shapes of the segment-id (packed sequence) tests —
TEST INFRASTRUCTURE ONLY; a plain helper shared by the CPU and GPU tests.

The reference is a dense masked softmax: fp32 inputs, fp64 arithmetic
inside (as tests/boundary_refs.py does for merges), pair (i, j) visible iff
``q_seg[i] == kv_seg[j]`` and, with ``causal``, ``j <= i``.  Its gradients
are the tile math of ``oracle.tile_bwd`` under the same mask.
tests/test_segments_cpu.py pins it to the golden-pinned oracle run per
document.  A row that sees no key has o = 0, lse = -inf and zero gradients.

The inputs make one-pair errors visible (cf. tests/boundary_inputs.py): at
every document boundary p (the first token of a document) key p-1 is hot
for query p and its V row is poisoned; in non-causal cases key p is hot
for query p-1 as well.  The gates are those of tests/test_gpu_parity.py,
through tests/boundary_refs.gates.
"""

import functools
import math

import torch

from .boundary_inputs import K_POISON, V_POISON  # noqa: F401 (re-exported)
from .gqa_cpu_provider import expand_kv, reduce_kv_grad

# The poisoned V rows are visible to their own document, so their size is
# part of every legitimate output: V_POISON (1e4, sized for rows no kernel
# may read) would put fp16 rounding of the legitimate terms far over the
# gates' atol.  K_POISON, the size boundary_inputs gives a leaked key, is
# O(10) and serves for both.
SEG_V_POISON = K_POISON

# ---- shapes (the smallest where the kernels can go wrong) ----------------
CAUSAL_S = 328
CAUSAL_CU = (0, 1, 33, 64, 200, 256, 257, 328)
RECT_SQ, RECT_SK = 96, 320


def ids_from_cu(cu, total):
    ids = torch.zeros(total, dtype=torch.int32)
    for d, (a, b) in enumerate(zip(cu[:-1], cu[1:])):
        ids[a:b] = d
    ids[cu[-1]:] = len(cu) - 1
    return ids


def rect_ids(b=2):
    """Independent id vectors of the rectangular non-causal tiles.  Keys of
    documents 5 and 6 are visible to no query; query id 9 is absent from
    the keys (rows 90..95 see nothing)."""
    q = ids_from_cu((0, 31, 60, 90, 96), RECT_SQ)      # ids 0, 1, 2, 3
    q[90:] = 9
    kv = torch.empty(RECT_SK, dtype=torch.int32)
    kv[:40] = 0
    kv[40:100] = 1
    kv[100:128] = 5
    kv[128:257] = 2
    kv[257:] = 6
    return q.expand(b, -1).contiguous(), kv.expand(b, -1).contiguous()


def mask_of(q_seg, kv_seg, causal):
    """[B, Sq, Sk] bool."""
    m = q_seg[:, :, None] == kv_seg[:, None, :]
    if causal:
        sq, sk = q_seg.shape[1], kv_seg.shape[1]
        assert sq == sk
        m = m & torch.ones(sq, sk, dtype=torch.bool).tril()
    return m


def seg_fwd(q, k, v, scale, causal, q_seg, kv_seg, mask=None):
    """(o fp32 [B,Sq,N,D], lse fp32 [B,N,Sq]); k/v may carry fewer heads.
    ``mask`` ([B,Sq,Sk] bool) replaces the mask built from the ids."""
    n = q.shape[2]
    qd = q.double().transpose(1, 2)
    kd = expand_kv(k, n).double().transpose(1, 2)
    vd = expand_kv(v, n).double().transpose(1, 2)
    s = qd @ kd.transpose(-1, -2) * scale
    m = (mask_of(q_seg, kv_seg, causal) if mask is None else mask)[:, None]
    s = s.masked_fill(~m, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - torch.where(lse.isinf(), torch.zeros_like(lse), lse)
                  .unsqueeze(-1))
    p = p.masked_fill(~m, 0.0)
    o = (p @ vd).transpose(1, 2)
    return o.float().contiguous(), lse.float().contiguous()


def seg_bwd(do, q, k, v, lse, scale, causal, q_seg, kv_seg, delta=None,
            o=None, mask=None):
    """(dq [.,.,N,D], dk, dv [.,.,Nk,D]) fp32: p = exp(s - lse) under the
    mask, ds = p (dp - delta) scale, as oracle.tile_bwd."""
    n, nk = q.shape[2], k.shape[2]
    qd = q.double().transpose(1, 2)
    kd = expand_kv(k, n).double().transpose(1, 2)
    vd = expand_kv(v, n).double().transpose(1, 2)
    gd = do.double().transpose(1, 2)
    if delta is None:
        delta = (o.double() * do.double()).sum(-1).transpose(1, 2)
    m = (mask_of(q_seg, kv_seg, causal) if mask is None else mask)[:, None]
    s = qd @ kd.transpose(-1, -2) * scale
    lsed = lse.double()
    lsed = torch.where(lsed.isinf(), torch.zeros_like(lsed), lsed)
    p = torch.exp(s.masked_fill(~m, float("-inf")) - lsed.unsqueeze(-1))
    p = p.masked_fill(~m, 0.0)
    dv = p.transpose(-1, -2) @ gd
    ds = p * (gd @ vd.transpose(-1, -2) - delta.double().unsqueeze(-1)) * scale
    dq = ds @ kd
    dk = ds.transpose(-1, -2) @ qd
    t = lambda x: x.transpose(1, 2).float().contiguous()
    return t(dq), reduce_kv_grad(t(dk), nk), reduce_kv_grad(t(dv), nk)


def boundaries(ids_row):
    """Positions p >= 1 with ids[p] != ids[p-1]."""
    return [p for p in range(1, ids_row.numel())
            if int(ids_row[p]) != int(ids_row[p - 1])]


def packed_inputs(b, sq, sk, n, nk, d, dtype, seed, kv_seg, causal):
    """(q, k, v, do): q rows of norm sqrt(d); at every boundary p of
    kv_seg[0] with p < sq, key p-1 scores about a = ln(sk) + 2 on query p
    (not visible to it) and v[p-1] is shifted by SEG_V_POISON; non-causal:
    key p also scores a on query p-1, and v[p] is shifted the other way."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, sq, n, d, generator=g)
    q = q * (math.sqrt(d) / q.norm(dim=-1, keepdim=True))
    k = torch.randn(b, sk, nk, d, generator=g)
    v = torch.randn(b, sk, nk, d, generator=g)
    do = torch.randn(b, sq, n, d, generator=g)
    a = math.log(max(sk, 2)) + 2.0
    qh = q[:, :, :: n // nk]
    for p in boundaries(kv_seg[0]):
        if p < sq:
            k[:, p - 1] += (a / math.sqrt(d)) * qh[:, p]
            v[:, p - 1] += SEG_V_POISON
            if not causal and p < sk:
                k[:, p] += (a / math.sqrt(d)) * qh[:, p - 1]
                v[:, p] -= SEG_V_POISON
    return tuple(t.to(dtype) for t in (q, k, v, do))


@functools.lru_cache(maxsize=None)
def causal_case(n, nk, d, dtype):
    """The causal tile of the issue: inputs, ids and reference, computed
    once and shared."""
    ids = ids_from_cu(CAUSAL_CU, CAUSAL_S).expand(2, -1).contiguous()
    q, k, v, do = packed_inputs(2, CAUSAL_S, CAUSAL_S, n, nk, d, dtype,
                                1234 + n + d, ids, True)
    return _with_ref(q, k, v, do, ids, ids, True)


@functools.lru_cache(maxsize=None)
def rect_case(n, nk, d, dtype):
    q_seg, kv_seg = rect_ids()
    q, k, v, do = packed_inputs(2, RECT_SQ, RECT_SK, n, nk, d, dtype,
                                4321 + n + d, kv_seg, False)
    return _with_ref(q, k, v, do, q_seg, kv_seg, False)


def _with_ref(q, k, v, do, q_seg, kv_seg, causal):
    sc = 1.0 / math.sqrt(q.shape[-1])
    o, lse = seg_fwd(q, k, v, sc, causal, q_seg, kv_seg)
    dq, dk, dv = seg_bwd(do, q, k, v, lse, sc, causal, q_seg, kv_seg, o=o)
    return dict(q=q, k=k, v=v, do=do, q_seg=q_seg, kv_seg=kv_seg,
                causal=causal, scale=sc, o=o, lse=lse, dq=dq, dk=dk, dv=dv)


def exceeds(actual, expected, gate):
    """Largest |actual - expected| / (atol + rtol |expected|): > 1 fails
    torch.testing.assert_close at that gate."""
    a, e = actual.double(), expected.double()
    both_inf = a.isinf() & e.isinf() & (a == e)
    err = (a - e).abs() / (gate["atol"] + gate["rtol"] * e.abs())
    err = torch.where(both_inf, torch.zeros_like(err), err)
    return float(torch.nan_to_num(err, nan=float("inf")).max())
