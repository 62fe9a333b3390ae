"""Multi-process (gloo, CPU) correctness of the ring orchestration.

Recreates the reference's integration test (test/test_burst.py:159-219) on
CPU: every rank builds the same seeded full sequence, runs single-process
eager attention as the oracle, chunks per rank (plain / zigzag / striped,
test_burst.py:44-58), runs burst_attn_func through the REAL orchestration
(interface + Ring over gloo) with the oracle tile provider injected, and
compares output and dq/dk/dv chunks.

This covers the N>1 product path (round structure, payload layouts, the
travelling-dq second ring, zigzag/striped bookkeeping) without a GPU —
the HIP tile itself is covered by tests/test_gpu_parity.py.
"""

import os

import pytest
import torch

import oracle
from oracle.partition import get_chunk

from .gloo_ranks import run_ranks

WORLD = 2
RTOL, ATOL = 1e-4, 1e-4


# max |error| allowed per tensor on the bf16-input case (rtol 0): twice what
# the ring code before the layouts shared one driver measured on this case,
# against the oracle on fp32 copies of the same bf16 inputs, larger of the
# two ranks (0.00390518, 0.0153975, 0.00770116, 0.0058302;
# profiles/ring_driver/README.md)
BF16_ATOL = {"o": 0.00781036, "dv": 0.030795, "dk": 0.01540232, "dq": 0.0116604}


def _worker(rank, world, causal, striped, optimize_bwd_comm, deterministic,
            dq_wire=None, dtype=torch.float32):
    if dq_wire is not None:
        os.environ["BA_DQ_WIRE"] = dq_wire
    from burst_attn_amd.tile import _set_tile_provider_for_testing
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped
    from .cpu_tile_provider import OracleTileProvider

    _set_tile_provider_for_testing(OracleTileProvider())

    b, s_local, n, d = 2, 64, 2, 64
    s = s_local * world
    g = torch.Generator().manual_seed(20240915)
    q = torch.randn(b, s, n, d, generator=g).to(dtype)
    k = torch.randn(b, s, n, d, generator=g).to(dtype)
    v = torch.randn(b, s, n, d, generator=g).to(dtype)
    do = torch.randn(b, s, n, d, generator=g).to(dtype)

    # the oracle computes in fp32 on fp32 copies of its inputs
    o_ref, dq_ref, dk_ref, dv_ref = oracle.ring_forward_backward_reference(
        q, k, v, do, None, causal
    )

    zig = causal and not striped
    ch = lambda t: get_chunk(t, 1, rank, world, zigzag=zig, striped=striped)
    qc = ch(q).requires_grad_()
    kc = ch(k).requires_grad_()
    vc = ch(v).requires_grad_()
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(qc, kc, vc, None, "cuda", causal, optimize_bwd_comm, deterministic)
    dq, dk, dv = torch.autograd.grad(o, (qc, kc, vc), ch(do))

    for name, got, ref in (("o", o, o_ref), ("dv", dv, dv_ref),
                           ("dk", dk, dk_ref), ("dq", dq, dq_ref)):
        assert got.dtype == dtype
        if dtype == torch.float32:
            tol = dict(rtol=RTOL, atol=ATOL)
        else:
            tol = dict(rtol=0, atol=BF16_ATOL[name])
            print(f"rank {rank} {name}: max |error| "
                  f"{(got.float() - ch(ref)).abs().max().item():.6g}")
        torch.testing.assert_close(got.float(), ch(ref), **tol)


@pytest.mark.parametrize("deterministic", [False])
@pytest.mark.parametrize("optimize_bwd_comm", [False, True])
@pytest.mark.parametrize("causal,striped", [
    (False, False),
    (True, False),   # zigzag
    (True, True),    # striped
    (False, True),   # striped layout, non-causal
])
def test_ring_matches_full_attention(causal, striped, optimize_bwd_comm, deterministic):
    run_ranks(_worker, WORLD, causal, striped, optimize_bwd_comm, deterministic)


def test_world_size_one_no_comm():
    """W=1 degenerates to one local tile — must work without any P2P."""
    import subprocess, sys
    code = r"""
import os, sys, torch
import torch.distributed as dist
sys.path.insert(0, os.getcwd())
# own rendezvous: a parent that already opened a process group exports its
# MASTER_PORT, and that port is still bound while the parent lives
os.environ["MASTER_ADDR"] = "127.0.0.1"
os.environ["MASTER_PORT"] = "29599"
dist.init_process_group("gloo", rank=0, world_size=1)
from burst_attn_amd.tile import _set_tile_provider_for_testing
from burst_attn_amd import burst_attn_func
from tests.cpu_tile_provider import OracleTileProvider
import oracle
_set_tile_provider_for_testing(OracleTileProvider())
g = torch.Generator().manual_seed(5)
q = torch.randn(1, 64, 2, 64, generator=g, requires_grad=True)
k = torch.randn(1, 64, 2, 64, generator=g, requires_grad=True)
v = torch.randn(1, 64, 2, 64, generator=g, requires_grad=True)
do = torch.randn(1, 64, 2, 64, generator=g)
o = burst_attn_func(q, k, v, None, "cuda", True)
dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
o_ref, dq_r, dk_r, dv_r = oracle.ring_forward_backward_reference(q, k, v, do, None, True)
torch.testing.assert_close(o, o_ref.to(o.dtype), rtol=1e-4, atol=1e-4)
torch.testing.assert_close(dq, dq_r, rtol=1e-4, atol=1e-4)
print("OK")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True,
                       text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("causal,striped", [(True, False), (True, True)])
def test_ring_odd_world_size(causal, striped):
    """W=3: odd ring size exercises the even/odd P2P ordering with two
    adjacent even ranks and non-power-of-two chunking."""
    run_ranks(_worker, 3, causal, striped, False, False, what="odd-ring")


@pytest.mark.parametrize("causal,striped", [(True, False), (True, True)])
def test_ring_fp32_dq_swap_path(causal, striped):
    """W=3 with BA_DQ_WIRE=fp32: the travelling dq hops by swapping fp32
    buffers instead of going through the wire buffers, on the flat ring
    (the double ring always swaps)."""
    run_ranks(_worker, 3, causal, striped, False, False, "fp32",
              what="dq-swap")


def test_ring_bf16_dq_wire_cast():
    """W=2 zigzag causal on bf16 inputs: the default wire path with a real
    cast of the fp32 travelling dq to the input dtype at every hop."""
    run_ranks(_worker, 2, True, False, False, False, None, torch.bfloat16,
              what="bf16-wire")
