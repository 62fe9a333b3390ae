"""Gates and oracle references of the boundary cases — TEST INFRASTRUCTURE
ONLY; a plain helper shared by tests/test_gpu_boundary.py and the CPU
tests, so that no test module imports another one's internals.

The gates are the ones tests/test_gpu_parity.py asserts, imported, not
restated.  The references are computed once on the CPU per (case, dtype),
shared by every test that names the case, and never modified.
"""

import functools
import math

import torch

import oracle

from . import boundary_inputs as bi
from .gqa_cpu_provider import expand_kv, reduce_kv_grad
from .test_gpu_parity import BWD_TOL, LSE_TOL, TOL


def gates(dtype, g):
    """The gate of each asserted output; dk/dv get G x atol
    (tests/test_gpu_gqa.py's rule for a sum of G per-head terms)."""
    b = BWD_TOL[dtype]
    kv = dict(rtol=b["rtol"], atol=g * b["atol"])
    return {"o": TOL[dtype], "lse": LSE_TOL, "dq": b, "dk": kv, "dv": kv}


def scale_of(case):
    return 1.0 / math.sqrt(case.d)


@functools.lru_cache(maxsize=None)
def inputs(case, dtype):
    return bi.make_inputs(case, dtype)


@functools.lru_cache(maxsize=None)
def round2_kv(case, dtype):
    return bi.round2_kv(case, dtype)


@functools.lru_cache(maxsize=None)
def fwd_ref(case, dtype):
    q, k, v, _ = inputs(case, dtype)
    return oracle.tile_fwd(q, expand_kv(k, case.n), expand_kv(v, case.n),
                           scale_of(case), case.causal)


@functools.lru_cache(maxsize=None)
def carry_ref(case, dtype):
    """(o, lse) of round 1 under the case's mask followed by round 2
    unmasked.  Unmasked round 1: the oracle tile on the concatenated keys.
    Causal round 1: oracle.tile_fwd has no mask for [tril | ones], so the
    two oracle tiles are merged with the oracle's own LSE merge
    (tests/test_boundary_inputs_cpu.py checks that against the eager
    softmax under the explicit mask)."""
    q, k, v, _ = inputs(case, dtype)
    k2, v2 = round2_kv(case, dtype)
    n = case.n
    if not case.causal:
        return oracle.tile_fwd(q, expand_kv(torch.cat([k, k2], 1), n),
                               expand_kv(torch.cat([v, v2], 1), n),
                               scale_of(case), False)
    o1, lse1 = fwd_ref(case, dtype)
    o2, lse2 = oracle.tile_fwd(q, expand_kv(k2, n), expand_kv(v2, n),
                               scale_of(case), False)
    o, lse = oracle.scale_out_lse(
        o1, lse1.transpose(-2, -1).unsqueeze(-1), o2, lse2)
    return o, lse.squeeze(-1).transpose(-2, -1).contiguous()


def _bns(lse):
    """[B,S,N,1] merged lse -> [B,N,S]."""
    return lse.squeeze(-1).transpose(-2, -1).contiguous()


def _merge_rows_from_1(o1, lse1, o2, lse2):
    """Rows 1.. of tile 1 merged with tile 2 (one row shorter); row 0 is
    tile 1 alone.  fp64 inside: a dominated round's lse gap overflows
    fp32's exp."""
    o, lse = o1.clone(), lse1.transpose(-2, -1).unsqueeze(-1).contiguous()
    om, lm = oracle.scale_out_lse(o[:, 1:].double(), lse[:, 1:].double(),
                                  o2.double(), lse2.double())
    o[:, 1:], lse[:, 1:] = om.float(), lm.float()
    return o, _bns(lse)


@functools.lru_cache(maxsize=None)
def shifted_ref(case, dtype):
    """(o, lse) of a fresh causal round on (k, v) followed by the striped
    ring's shifted round on round2_kv: rows 1.. against keys ..-1 under
    the causal mask, merged into state rows 1.. ."""
    assert case.causal and case.sq >= 2
    q, _, _, _ = inputs(case, dtype)
    k2, v2 = round2_kv(case, dtype)
    o1, lse1 = fwd_ref(case, dtype)
    o2, lse2 = oracle.tile_fwd(q[:, 1:], expand_kv(k2, case.n)[:, :-1],
                               expand_kv(v2, case.n)[:, :-1], scale_of(case),
                               True)
    return _merge_rows_from_1(o1, lse1, o2, lse2)


@functools.lru_cache(maxsize=None)
def merged_bwd_ref(case, dtype):
    """(dq, dk, dv, dk2, dv2) of the two rounds of shifted_ref, each tile
    differentiated under the MERGED lse and delta = rowsum(o_merged * dO),
    as in the ring: a tile's P is then a fragment of a row.  dq sums both
    tiles; dk2/dv2 belong to round2_kv, their last row stays zero."""
    q, k, v, do = inputs(case, dtype)
    k2, v2 = round2_kv(case, dtype)
    n, nk, sc = case.n, case.nk, scale_of(case)
    o, lse = shifted_ref(case, dtype)
    delta = (o * do.float()).sum(-1).transpose(1, 2).contiguous()
    dq, dk, dv = oracle.tile_bwd(do, q, expand_kv(k, n), expand_kv(v, n),
                                 lse, sc, True, softmax_d=delta)
    dq2, dk2, dv2 = oracle.tile_bwd(
        do[:, 1:], q[:, 1:], expand_kv(k2, n)[:, :-1],
        expand_kv(v2, n)[:, :-1], lse[:, :, 1:], sc, True,
        softmax_d=delta[:, :, 1:])
    dq[:, 1:] += dq2
    pad = lambda g: torch.cat(
        [reduce_kv_grad(g, nk), torch.zeros(case.b, 1, nk, case.d)], 1)
    return (dq, reduce_kv_grad(dk, nk), reduce_kv_grad(dv, nk), pad(dk2),
            pad(dv2))


@functools.lru_cache(maxsize=None)
def dominated_kv(case, dtype, which):
    return bi.dominated_kv(case, dtype, which)


@functools.lru_cache(maxsize=None)
def dominated_ref(case, dtype, which):
    """(o, lse) of a fresh causal round on (k, v) followed by a causal
    carry-in round on dominated_kv: the oracle merge of the two oracle
    tiles."""
    q, _, _, _ = inputs(case, dtype)
    k2, v2 = dominated_kv(case, dtype, which)
    o1, lse1 = fwd_ref(case, dtype)
    o2, lse2 = oracle.tile_fwd(q, expand_kv(k2, case.n),
                               expand_kv(v2, case.n), scale_of(case), True)
    o, lse = oracle.scale_out_lse(
        o1.double(), lse1.transpose(-2, -1).unsqueeze(-1).double(), o2,
        lse2.double())
    return o.float(), _bns(lse.float())


@functools.lru_cache(maxsize=None)
def bwd_ref(case, dtype):
    q, k, v, do = inputs(case, dtype)
    ke, ve = expand_kv(k, case.n), expand_kv(v, case.n)
    o, lse = fwd_ref(case, dtype)
    dq, dk, dv = oracle.tile_bwd(do, q, ke, ve, lse, scale_of(case),
                                 case.causal, o=o)
    return dq, reduce_kv_grad(dk, case.nk), reduce_kv_grad(dv, case.nk)
