"""GPU tests of grouped-query attention (GQA/MQA): k/v with Nk < N heads.

Reference for every numeric case: the CPU oracle on K/V expanded with
``repeat_interleave(G, dim=2)`` and dk/dv reduced over each group in fp32
(tests/gqa_cpu_provider.py).  Tolerances are the existing gates of
test_gpu_parity.py / test_gpu_ring_sim.py; dk/dv get G x the backward atol
because each is a sum of G per-head terms that are individually held to
that atol.

The bitwise cases compare the grouped kernels against G calls of the
equal-heads path on strided head views (``q[:, :, g::G]`` ...): the
arithmetic of a query head does not depend on where its K/V pointer came
from, so any difference there is an indexing bug.
"""

import functools
import math
import os

import pytest
import torch

import oracle

from .gqa_cpu_provider import expand_kv, gqa_full_reference, reduce_kv_grad
from .ring_sim import simulate_ring
from .test_gpu_parity import BWD_TOL, TOL

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
LSE_TOL = dict(rtol=1e-3, atol=2e-2)  # test_gpu_parity's lse gate


def _ext():
    from burst_attn_amd._ext import load_extension

    return load_extension()


def _kv_tol(dtype, g):
    t = BWD_TOL[dtype]
    return dict(rtol=t["rtol"], atol=g * t["atol"])


@functools.lru_cache(maxsize=None)
def _inputs(b, sq, sk, n, nk, d, dtype):
    """Seeded (q, k, v, do) on CPU in `dtype` — shared, never modified."""
    g = torch.Generator().manual_seed(1234 + 7 * sq + 3 * sk + n + nk + d)
    mk = lambda s, h: torch.randn(b, s, h, d, generator=g).to(dtype)
    return mk(sq, n), mk(sk, nk), mk(sk, nk), mk(sq, n)


@functools.lru_cache(maxsize=None)
def _fwd_ref(b, sq, sk, n, nk, d, dtype, causal):
    q, k, v, _ = _inputs(b, sq, sk, n, nk, d, dtype)
    return oracle.tile_fwd(q, expand_kv(k, n), expand_kv(v, n),
                           1.0 / math.sqrt(d), causal)


@functools.lru_cache(maxsize=None)
def _bwd_ref(b, sq, sk, n, nk, d, dtype, causal):
    q, k, v, do = _inputs(b, sq, sk, n, nk, d, dtype)
    scale = 1.0 / math.sqrt(d)
    ke, ve = expand_kv(k, n), expand_kv(v, n)
    o, lse = oracle.tile_fwd(q, ke, ve, scale, causal)
    dq, dk, dv = oracle.tile_bwd(do, q, ke, ve, lse, scale, causal, o=o)
    return dq, reduce_kv_grad(dk, nk), reduce_kv_grad(dv, nk)


def _gpu(*ts):
    return tuple(t.cuda() for t in ts)


# (b, sq, sk, N, Nk, d)
FWD_SHAPES = [
    (2, 256, 256, 4, 2, 128),  # B=2: a batch / KV-head stride mix-up shows
    (1, 256, 256, 6, 2, 128),  # G=3, not a power of two
    (1, 300, 300, 4, 1, 64),   # MQA, ragged, d=64
    (1, 96, 320, 4, 2, 128),   # sq != sk: non-causal only
]
FWD_CASES = [(s, c) for s in FWD_SHAPES for c in (False, True)
             if not (c and s[1] != s[2])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,causal", FWD_CASES)
def test_fwd_tile_vs_expanded_oracle(shape, causal, dtype):
    b, sq, sk, n, nk, d = shape
    q, k, v, _ = _gpu(*_inputs(*shape, dtype))
    o, lse = _ext().attn_fwd(q, k, v, 1.0 / math.sqrt(d), causal)
    o_ref, lse_ref = _fwd_ref(*shape, dtype, causal)
    assert o.shape == (b, sq, n, d) and lse.shape == (b, n, sq)
    torch.testing.assert_close(o.cpu(), o_ref, **TOL[dtype])
    torch.testing.assert_close(lse.cpu(), lse_ref, **LSE_TOL)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fwd_accum_row_offset_window(dtype):
    """Carry-in accumulator with Nk-head K/V, including the zigzag half
    window (row_offset): rows [:half] saw kv [:s], rows [half:] all of it."""
    from burst_attn_amd.tile import HipTileProvider

    P = HipTileProvider()
    b, s, n, nk, d = 2, 256, 4, 2, 128
    q, k, v, _ = _gpu(*_inputs(b, s, 2 * s, n, nk, d, dtype))
    scale = 1.0 / math.sqrt(d)
    half = s // 2
    st = P.fwd_accum(None, q, k[:, :s], v[:, :s], scale, False)
    st = P.fwd_accum(st, q[:, half:], k[:, s:], v[:, s:], scale, False,
                     row_offset=half)
    o, lse = P.fwd_finalize(st, dtype)
    qc, kc, vc, _ = _inputs(b, s, 2 * s, n, nk, d, dtype)
    ke, ve = expand_kv(kc, n), expand_kv(vc, n)
    o_top, lse_top = oracle.tile_fwd(qc[:, :half], ke[:, :s], ve[:, :s], scale, False)
    o_bot, lse_bot = oracle.tile_fwd(qc[:, half:], ke, ve, scale, False)
    torch.testing.assert_close(o[:, :half].float().cpu(), o_top, **TOL[dtype])
    torch.testing.assert_close(o[:, half:].float().cpu(), o_bot, **TOL[dtype])
    torch.testing.assert_close(lse[:, :, :half].cpu(), lse_top, **LSE_TOL)
    torch.testing.assert_close(lse[:, :, half:].cpu(), lse_bot, **LSE_TOL)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fwd_striped_shift_views(dtype):
    """The striped ring's one-token shift: q[:, 1:] vs k[:, :-1] views."""
    shape = (2, 256, 256, 4, 2, 128)
    n, d = shape[3], shape[5]
    q, k, v, _ = _gpu(*_inputs(*shape, dtype))
    scale = 1.0 / math.sqrt(d)
    o, lse = _ext().attn_fwd(q[:, 1:], k[:, :-1], v[:, :-1], scale, True)
    qc, kc, vc, _ = _inputs(*shape, dtype)
    o_ref, lse_ref = oracle.tile_fwd(
        qc[:, 1:], expand_kv(kc, n)[:, :-1], expand_kv(vc, n)[:, :-1], scale, True)
    torch.testing.assert_close(o.cpu(), o_ref, **TOL[dtype])
    torch.testing.assert_close(lse.cpu(), lse_ref, **LSE_TOL)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", [(2, 320, 320, 4, 2, 128),
                                   (1, 256, 256, 6, 2, 128),
                                   (1, 200, 200, 4, 1, 64)])
def test_grouped_fwd_and_dq_bitwise_vs_per_head_calls(shape, causal, dtype):
    b, s, _, n, nk, d = shape
    G = n // nk
    ext = _ext()
    q, k, v, do = _gpu(*_inputs(*shape, dtype))
    scale = 1.0 / math.sqrt(d)
    o, lse = ext.attn_fwd(q, k, v, scale, causal)
    delta = ext.attn_bwd_preprocess(o.to(dtype), do)
    dq, dk, dv = ext.attn_bwd(do, q, k, v, delta, lse, scale, causal, True)
    dq_c = torch.zeros_like(dq)
    dk_c, dv_c = torch.zeros_like(dk), torch.zeros_like(dv)
    for g in range(G):
        # the equal-heads path: Nk query heads against the Nk kv heads
        o_g, lse_g = ext.attn_fwd(q[:, :, g::G], k, v, scale, causal)
        assert torch.equal(o_g, o[:, :, g::G]), f"o differs for member {g}"
        assert torch.equal(lse_g, lse[:, g::G]), f"lse differs for member {g}"
        ext.attn_bwd_accum(do[:, :, g::G], q[:, :, g::G], k, v, delta[:, g::G],
                           lse[:, g::G], scale, causal, True,
                           dq_c[:, :, g::G], dk_c, dv_c)
    assert torch.equal(dq, dq_c), "dq differs from the per-head calls"
    # dk/dv: the G launches add the same per-head terms in another order
    # (one fp32 read-modify-write per head instead of one per group), so
    # they are not bitwise; hold them to the backward gate for a G-term sum
    torch.testing.assert_close(dk, dk_c, **_kv_tol(dtype, G))
    torch.testing.assert_close(dv, dv_c, **_kv_tol(dtype, G))


# (b, sq, sk, N, Nk, d)
BWD_SHAPES = [
    (1, 256, 256, 4, 2, 128),
    (2, 320, 320, 4, 2, 128),  # causal: 2nd kv workgroup has t0 > 0; ragged
    (1, 128, 320, 4, 1, 128),  # MQA, sq != sk: non-causal only
    (1, 200, 200, 6, 2, 64),
]
BWD_CASES = [(s, c) for s in BWD_SHAPES for c in (False, True)
             if not (c and s[1] != s[2])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,causal", BWD_CASES)
def test_bwd_tile_vs_expanded_oracle(shape, causal, dtype):
    b, sq, sk, n, nk, d = shape
    ext = _ext()
    q, k, v, do = _gpu(*_inputs(*shape, dtype))
    scale = 1.0 / math.sqrt(d)
    o, lse = ext.attn_fwd(q, k, v, scale, causal)
    delta = ext.attn_bwd_preprocess(o.to(dtype), do)
    dq, dk, dv = ext.attn_bwd(do, q, k, v, delta, lse, scale, causal, False)
    assert dq.shape == (b, sq, n, d)
    assert dk.shape == (b, sk, nk, d) and dv.shape == (b, sk, nk, d)
    dq_r, dk_r, dv_r = _bwd_ref(*shape, dtype, causal)
    kv_tol = _kv_tol(dtype, n // nk)
    torch.testing.assert_close(dv.cpu(), dv_r, **kv_tol)
    torch.testing.assert_close(dk.cpu(), dk_r, **kv_tol)
    torch.testing.assert_close(dq.cpu(), dq_r, **BWD_TOL[dtype])


# One fp32 add per element per call (the epilogue's read-add-write), so the
# accumulate identities hold to fp32 roundoff of values of magnitude <~ 1e2:
# a few ulp (2^-23 relative) plus an absolute floor for cancelling sums.
ACC_TOL = dict(rtol=1e-6, atol=1e-5)


def _bwd_setup(shape, dtype, causal):
    b, sq, sk, n, nk, d = shape
    ext = _ext()
    q, k, v, do = _gpu(*_inputs(*shape, dtype))
    scale = 1.0 / math.sqrt(d)
    o, lse = ext.attn_fwd(q, k, v, scale, causal)
    delta = ext.attn_bwd_preprocess(o.to(dtype), do)
    return ext, q, k, v, do, delta, lse, scale


def _prefill(like_shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(like_shape, generator=g).cuda()


@pytest.mark.parametrize("causal", [False, True])
def test_bwd_accum_prefilled_and_twice(causal):
    shape = (2, 320, 320, 4, 2, 128)
    ext, q, k, v, do, delta, lse, scale = _bwd_setup(shape, torch.float16, causal)
    args = (do, q, k, v, delta, lse, scale, causal, True)
    # one call's contribution, twice from zero: summed on the host below
    c1 = ext.attn_bwd(*args)
    c2 = ext.attn_bwd(*args)
    pre = [_prefill(c.shape, 300 + i) for i, c in enumerate(c1)]
    acc = [p.clone() for p in pre]
    ext.attn_bwd_accum(*args, *acc)
    for a, p, x in zip(acc, pre, c1):
        torch.testing.assert_close(a, p + x, **ACC_TOL)
    ext.attn_bwd_accum(*args, *acc)
    for a, p, x, y in zip(acc, pre, c1, c2):
        torch.testing.assert_close(a, p + x + y, **ACC_TOL)


def test_bwd_accum_into_ring_views():
    """The zigzag rounds' targets: dk/dv[:, :half] with k/v[:, :half], and
    dq[:, half:] with the travelling q's second half."""
    shape = (2, 320, 320, 4, 2, 128)
    b, s, _, n, nk, d = shape
    half = s // 2
    ext, q, k, v, do, delta, lse, scale = _bwd_setup(shape, torch.float16, False)
    pre = [_prefill((b, s, h, d), 400 + i) for i, h in enumerate((n, nk, nk))]

    # kv_half: all q rows vs my kv first half
    args = (do, q, k[:, :half], v[:, :half], delta, lse, scale, False, True)
    cq, ck, cv = ext.attn_bwd(*args)
    dq, dk, dv = (p.clone() for p in pre)
    ext.attn_bwd_accum(*args, dq, dk[:, :half], dv[:, :half])
    torch.testing.assert_close(dq, pre[0] + cq, **ACC_TOL)
    torch.testing.assert_close(dk[:, :half], pre[1][:, :half] + ck, **ACC_TOL)
    torch.testing.assert_close(dv[:, :half], pre[2][:, :half] + cv, **ACC_TOL)
    assert torch.equal(dk[:, half:], pre[1][:, half:]), "dk second half touched"
    assert torch.equal(dv[:, half:], pre[2][:, half:]), "dv second half touched"

    # q_half: q second half vs my full kv
    args = (do[:, half:], q[:, half:], k, v, delta[:, :, half:],
            lse[:, :, half:], scale, False, True)
    cq, ck, cv = ext.attn_bwd(*args)
    dq, dk, dv = (p.clone() for p in pre)
    ext.attn_bwd_accum(*args, dq[:, half:], dk, dv)
    torch.testing.assert_close(dq[:, half:], pre[0][:, half:] + cq, **ACC_TOL)
    assert torch.equal(dq[:, :half], pre[0][:, :half]), "dq first half touched"
    torch.testing.assert_close(dk, pre[1] + ck, **ACC_TOL)
    torch.testing.assert_close(dv, pre[2] + cv, **ACC_TOL)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gqa_backward_bitwise_deterministic(dtype):
    shape = (2, 320, 320, 6, 2, 128)
    ext, q, k, v, do, delta, lse, scale = _bwd_setup(shape, dtype, True)
    a = ext.attn_bwd(do, q, k, v, delta, lse, scale, True, True)
    b_ = ext.attn_bwd(do, q, k, v, delta, lse, scale, True, True)
    for x, y in zip(a, b_):
        assert torch.equal(x, y), "GQA backward is not bitwise deterministic"


@pytest.mark.parametrize("knob,value", [("BA_BWD_FUSED", "1"),
                                        ("BA_BWD_FUSED", "2"),
                                        ("BA_BWD_DK_FLIP", "1")])
def test_experiment_plans_reject_gqa(knob, value, monkeypatch):
    """The bwd_dkq_kernel experiment plans are equal-heads only: with
    Nk != N they must fail naming the knob, never fall back or mis-index."""
    shape = (1, 256, 256, 4, 2, 128)
    ext, q, k, v, do, delta, lse, scale = _bwd_setup(shape, torch.float16, False)
    monkeypatch.setenv(knob, value)
    with pytest.raises(RuntimeError, match=f"{knob}={value}"):
        ext.attn_bwd(do, q, k, v, delta, lse, scale, False, False)


class _GpuProvider:
    """simulate_ring's provider contract over the HIP kernels (the wrapper
    pattern of test_gpu_ring_sim.py)."""

    def __init__(self):
        from burst_attn_amd.tile import HipTileProvider

        self._p = HipTileProvider()

    def fwd(self, q, k, v, scale, causal):
        return self._p.fwd(q, k, v, scale, causal)

    def bwd_preprocess(self, o, do):
        return self._p.bwd_preprocess(o, do)

    def bwd(self, do, q, k, v, delta, lse, scale, causal, det):
        return self._p.bwd(do, q, k, v, delta, lse, scale, causal, det)

    def merge(self, o, lse, o_i, lse_i):
        return self._p.merge(o, lse, o_i, lse_i)


@functools.lru_cache(maxsize=None)
def _ring_ref(causal):
    b, s, n, nk, d = 1, 1024, 4, 2, 128
    q, k, v, do = _inputs(b, s, s, n, nk, d, torch.float16)
    return gqa_full_reference(q, k, v, do, 1.0 / math.sqrt(d), causal)


@pytest.mark.parametrize("causal,striped", [
    (False, False), (True, False), (True, True), (False, True),
])
def test_gqa_ring_sim_w4_gpu(causal, striped):
    W = 4
    b, s, n, nk, d = 1, 256 * W, 4, 2, 128
    q, k, v, do = _gpu(*_inputs(b, s, s, n, nk, d, torch.float16))
    scale = 1.0 / math.sqrt(d)
    o, dq, dk, dv = simulate_ring(_GpuProvider(), q, k, v, do, W, scale,
                                  causal, striped)
    assert dk.shape == k.shape and dv.shape == v.shape
    o_ref, dq_r, dk_r, dv_r = _ring_ref(causal)
    # test_gpu_ring_sim.py's gates: o is its fp16 TOL; its btol is a
    # literal inside that test's body, so it can only be restated here
    tol = TOL[torch.float16]
    btol = dict(rtol=5e-3, atol=3e-2)
    kv_tol = dict(rtol=btol["rtol"], atol=(n // nk) * btol["atol"])
    torch.testing.assert_close(o.float().cpu(), o_ref, **tol)
    torch.testing.assert_close(dv.float().cpu(), dv_r, **kv_tol)
    torch.testing.assert_close(dk.float().cpu(), dk_r, **kv_tol)
    torch.testing.assert_close(dq.float().cpu(), dq_r, **btol)


@pytest.mark.parametrize("striped", [False, True])
@pytest.mark.parametrize("causal", [False, True])
def test_gqa_interface_end_to_end_single_rank(causal, striped):
    """burst_attn_func autograd cycle with Nk-head k/v on one GPU (W=1)."""
    import torch.distributed as dist

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29714")
        dist.init_process_group("nccl", rank=0, world_size=1)
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    b, s, n, nk, d = 2, 512, 4, 2, 128
    qc, kc, vc, doc = _inputs(b, s, s, n, nk, d, torch.float16)
    q, k, v = (t.cuda().requires_grad_() for t in (qc, kc, vc))
    do = doc.cuda()
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(q, k, v, None, "cuda", causal)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
    assert dk.shape == k.shape and dv.shape == v.shape and dq.shape == q.shape
    assert dk.dtype == k.dtype
    o_ref, dq_r, dk_r, dv_r = gqa_full_reference(qc, kc, vc, doc, None, causal)
    # test_interface_end_to_end_single_rank's gates (fp16 TOL / BWD_TOL)
    tol, btol = TOL[torch.float16], BWD_TOL[torch.float16]
    kv_tol = dict(rtol=btol["rtol"], atol=(n // nk) * btol["atol"])
    torch.testing.assert_close(o.float().cpu(), o_ref, **tol)
    torch.testing.assert_close(dv.float().cpu(), dv_r, **kv_tol)
    torch.testing.assert_close(dk.float().cpu(), dk_r, **kv_tol)
    torch.testing.assert_close(dq.float().cpu(), dq_r, **btol)
