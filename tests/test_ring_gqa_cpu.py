"""Grouped-query attention through the ring orchestration on CPU (gloo).

Same structure as tests/test_ring_cpu.py, with K/V carrying Nk < N heads
and the GQA oracle provider (tests/gqa_cpu_provider.py) injected.  The
reference is the equal-heads oracle on K/V expanded with
``repeat_interleave(G, dim=2)``, dk/dv reduced over each group in fp32.

Also pins that K/V travel the ring UNEXPANDED: the provider records the
head count of every K/V tile it is handed, and from the second round on
those tensors are what came over the wire.
"""

import os

import pytest
import torch

from oracle.partition import get_chunk

from .gloo_ranks import run_ranks
from .test_ring_cpu import ATOL, RTOL


def _worker(rank, world, causal, striped, optimize_bwd_comm, nk):
    from burst_attn_amd.tile import _set_tile_provider_for_testing
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped
    from .gqa_cpu_provider import GqaOracleTileProvider, gqa_full_reference

    P = GqaOracleTileProvider()
    _set_tile_provider_for_testing(P)

    b, s_local, n, d = 2, 64, 4, 64
    s = s_local * world
    g = torch.Generator().manual_seed(20250611)
    q = torch.randn(b, s, n, d, generator=g)
    k = torch.randn(b, s, nk, d, generator=g)
    v = torch.randn(b, s, nk, d, generator=g)
    do = torch.randn(b, s, n, d, generator=g)

    o_ref, dq_ref, dk_ref, dv_ref = gqa_full_reference(q, k, v, do, None,
                                                       causal)

    zig = causal and not striped
    ch = lambda t: get_chunk(t, 1, rank, world, zigzag=zig, striped=striped)
    qc = ch(q).requires_grad_()
    kc = ch(k).requires_grad_()
    vc = ch(v).requires_grad_()
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(qc, kc, vc, None, "cuda", causal, optimize_bwd_comm, False)
    dq, dk, dv = torch.autograd.grad(o, (qc, kc, vc), ch(do))

    assert dk.shape == kc.shape and dv.shape == vc.shape
    assert dq.shape == qc.shape
    torch.testing.assert_close(o, ch(o_ref), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(dv, ch(dv_ref), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(dk, ch(dk_ref), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(dq, ch(dq_ref), rtol=RTOL, atol=ATOL)
    # unexpanded on the wire: one tile call per round, and the K/V of
    # every round after the first (received over the ring) has Nk heads
    assert len(P.fwd_kv_heads) == world and len(P.bwd_kv_heads) == world
    assert all(h == (nk, nk) for h in P.fwd_kv_heads[1:]), P.fwd_kv_heads
    assert all(h == (nk, nk) for h in P.bwd_kv_heads), P.bwd_kv_heads


def _spawn(world, causal, striped, optimize_bwd_comm, nk):
    run_ranks(_worker, world, causal, striped, optimize_bwd_comm, nk,
              what="GQA ring")


@pytest.mark.parametrize("optimize_bwd_comm", [False, True])
@pytest.mark.parametrize("causal,striped", [
    (False, False),
    (True, False),   # zigzag
    (True, True),    # striped
    (False, True),   # striped layout, non-causal
])
def test_gqa_ring_matches_expanded_attention(causal, striped, optimize_bwd_comm):
    _spawn(2, causal, striped, optimize_bwd_comm, nk=2)


def test_mqa_ring_odd_world_size():
    """W=3, non-causal, one KV head shared by all four query heads."""
    _spawn(3, False, False, False, nk=1)


# ---- interface validation ----------------------------------------------
# The head checks run before any ring or tile work, so the raising cases
# need neither a process group nor a provider.

def _qkv(n, nk, nv=None, d=64, dv=None):
    g = torch.Generator().manual_seed(3)
    q = torch.randn(1, 32, n, d, generator=g)
    k = torch.randn(1, 32, nk, d, generator=g)
    v = torch.randn(1, 32, nk if nv is None else nv, d if dv is None else dv,
                    generator=g)
    return q, k, v


@pytest.mark.parametrize("striped", [False, True])
def test_heads_not_divisible_raises(striped):
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    func = burst_attn_func_striped if striped else burst_attn_func
    q, k, v = _qkv(4, 3)
    with pytest.raises(ValueError, match=r"N=4.*Nk=3"):
        func(q, k, v, None, "cuda", False)


@pytest.mark.parametrize("striped", [False, True])
def test_kv_head_counts_differ_raises(striped):
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    func = burst_attn_func_striped if striped else burst_attn_func
    q, k, v = _qkv(4, 2, nv=4)
    with pytest.raises(ValueError, match=r"Nk=2.*N=4"):
        func(q, k, v, None, "cuda", False)


def test_head_dim_differs_raises():
    from burst_attn_amd import burst_attn_func

    q, k, v = _qkv(4, 2, dv=32)
    with pytest.raises(ValueError, match=r"head_dim.*N=4.*Nk=2"):
        burst_attn_func(q, k, v, None, "cuda", False)


def test_equal_heads_takes_todays_path():
    """Nk == N through the GQA provider at W=1: the tiles see N-head K/V and
    the result is the plain equal-heads oracle's.  Own process: the group
    must not leak into this one."""
    import subprocess, sys
    code = r"""
import os, sys, torch
import torch.distributed as dist
sys.path.insert(0, os.getcwd())
os.environ["MASTER_ADDR"] = "127.0.0.1"
os.environ["MASTER_PORT"] = "29650"
dist.init_process_group("gloo", rank=0, world_size=1)
from burst_attn_amd.tile import _set_tile_provider_for_testing
from burst_attn_amd import burst_attn_func
from tests.gqa_cpu_provider import GqaOracleTileProvider
import oracle
P = GqaOracleTileProvider()
_set_tile_provider_for_testing(P)
g = torch.Generator().manual_seed(5)
q = torch.randn(1, 64, 4, 64, generator=g, requires_grad=True)
k = torch.randn(1, 64, 4, 64, generator=g, requires_grad=True)
v = torch.randn(1, 64, 4, 64, generator=g, requires_grad=True)
do = torch.randn(1, 64, 4, 64, generator=g)
o = burst_attn_func(q, k, v, None, "cuda", True)
dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
assert P.fwd_kv_heads == [(4, 4)] and P.bwd_kv_heads == [(4, 4)]
o_ref, dq_r, dk_r, dv_r = oracle.ring_forward_backward_reference(q, k, v, do, None, True)
for a, b in ((o, o_ref), (dq, dq_r), (dk, dk_r), (dv, dv_r)):
    torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)
print("OK")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True,
                       text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
