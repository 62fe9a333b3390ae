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


@functools.lru_cache(maxsize=None)
def bwd_ref(case, dtype):
    q, k, v, do = inputs(case, dtype)
    ke, ve = expand_kv(k, case.n), expand_kv(v, case.n)
    o, lse = fwd_ref(case, dtype)
    dq, dk, dv = oracle.tile_bwd(do, q, ke, ve, lse, scale_of(case),
                                 case.causal, o=o)
    return dq, reduce_kv_grad(dk, case.nk), reduce_kv_grad(dv, case.nk)
