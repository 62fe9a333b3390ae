"""Logit soft-capping: the cap form of the tile kernels against plain fp64
attention with the one line ``s = softcap * tanh(s / softcap)`` added.

Reference: fp64 on the CPU, gradients by autograd through it, cached per
(shape, d, dtype, cap).  Gates: ``boundary_refs.gates``, i.e. TOL, BWD_TOL and
LSE_TOL of tests/test_gpu_parity.py, unchanged.

Inputs: randn with k scaled by 2, so the scaled scores have a standard
deviation of about 2: at cap 1.5 both the linear and the saturated range of
tanh are hit, at cap 30 the range near zero.  328 = 256 + 64 + 8 rows put a
seam on the 32-row wave, the 64-row tile, the 128- and 256-row blocks and a
ragged tail.  The causal cases at cap 1.5 are the ones a mask applied before
the tanh fails: a masked key would keep the weight e^-1.5 against at most
e^1.5 of a visible one, and row 0 has 327 masked keys next to its one key.
"""

import functools
import math

import pytest
import torch

from . import ring_rounds as rr
from .boundary_refs import gates

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16],
                                 ids=lambda t: str(t).split(".")[-1])
# (b, sq, sk, n, nk, causal)
FULL = (1, 328, 328, 4, 2, False)
CAUSAL = (1, 328, 328, 4, 2, True)
SENTINEL = 7.5


def _P():
    from burst_attn_amd.tile import HipTileProvider

    return HipTileProvider()


@functools.lru_cache(maxsize=None)
def _inputs(shape, d, dtype):
    b, sq, sk, n, nk, _ = shape
    g = torch.Generator().manual_seed(3000 + d + sq + 7 * sk + n)
    q, k, v, do = (torch.randn(b, s_, h, d, generator=g)
                   for s_, h in ((sq, n), (sk, nk), (sk, nk), (sq, n)))
    return tuple(t.to(dtype) for t in (q, 2 * k, v, do))


@functools.lru_cache(maxsize=None)
def _ref(shape, d, dtype, cap):
    """(o, lse [B,N,S], dq, dk, dv) of soft-capped attention in fp64."""
    n, nk, causal = shape[3], shape[4], shape[5]
    q, k, v, do = (t.double() for t in _inputs(shape, d, dtype))
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    ke, ve = (t.repeat_interleave(n // nk, dim=2) for t in (k, v))
    s = torch.einsum("bqnd,bknd->bnqk", q, ke) / math.sqrt(d)
    s = cap * torch.tanh(s / cap)
    if causal:
        s = s.masked_fill(~torch.ones(s.shape[-2:], dtype=torch.bool).tril(),
                          -math.inf)
    o = torch.einsum("bnqk,bknd->bqnd", torch.softmax(s, -1), ve)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
    return dict(zip(("o", "lse", "dq", "dk", "dv"),
                    (t.detach().float()
                     for t in (o, torch.logsumexp(s, -1), dq, dk, dv))))


def _check(got, ref, shape, dtype, names=("o", "lse", "dq", "dk", "dv")):
    gate = gates(dtype, shape[3] // shape[4])
    for name in names:
        torch.testing.assert_close(
            got[name].float().cpu(), ref[name], **gate[name],
            msg=lambda m, name=name: f"{name}: {m}")


def _fwd_bwd(p, shape, d, dtype, cap):
    q, k, v, do = (t.cuda() for t in _inputs(shape, d, dtype))
    scale, causal = 1.0 / math.sqrt(d), shape[5]
    o, lse = p.fwd(q, k, v, scale, causal, softcap=cap)
    delta = p.bwd_preprocess(o.to(dtype), do)
    dq, dk, dv = p.bwd(do, q, k, v, delta, lse, scale, causal, True,
                       softcap=cap)
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


# ---- 1. tiles ---------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("cap", [1.5, 30.0])
@pytest.mark.parametrize("heads", [(2, 2), (4, 2)], ids=str)
@pytest.mark.parametrize("b,sq,sk,causal", [
    (1, 328, 328, True), (2, 328, 328, False), (1, 96, 320, False)])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_tile_fwd_bwd(d, b, sq, sk, causal, heads, cap, dtype):
    shape = (b, sq, sk, *heads, causal)
    _check(_fwd_bwd(_P(), shape, d, dtype, cap), _ref(shape, d, dtype, cap),
           shape, dtype)


# ---- 2. carry-in --------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("d", [128, 256])
def test_carry_in_two_rounds(d, dtype):
    """Two rounds over the halves of the keys, then finalize, against the
    joint reference; started from fwd_empty_state the same, bit for bit."""
    p, h, cap, scale = _P(), 168, 1.5, 1.0 / math.sqrt(d)
    q, k, v, _ = (t.cuda() for t in _inputs(FULL, d, dtype))
    halves = (slice(None, h), slice(h, None))
    st, st0 = None, p.fwd_empty_state(q)
    for sl in halves:
        st = p.fwd_accum(st, q, k[:, sl], v[:, sl], scale, False, softcap=cap)
        st0 = p.fwd_accum(st0, q, k[:, sl], v[:, sl], scale, False,
                          softcap=cap)
    o, lse = p.fwd_finalize(st, dtype)
    _check(dict(o=o, lse=lse), _ref(FULL, d, dtype, cap), FULL, dtype,
           ("o", "lse"))
    for a, b2 in zip(st, st0):
        assert torch.equal(a, b2)


# ---- 3. the ring's rounds on one GPU ----------------------------------------

class _Capped:
    """A provider whose four tile calls carry ``softcap``."""

    def __init__(self, p, cap):
        self._p, self._cap = p, cap

    def __getattr__(self, name):
        f = getattr(self._p, name)
        if name in ("fwd", "fwd_accum", "bwd", "bwd_accum"):
            return functools.partial(f, softcap=self._cap)
        return f


@pytest.mark.parametrize("d,dtype", [(128, torch.float16),
                                     (256, torch.bfloat16)])
@pytest.mark.parametrize("layout", ["zigzag", "striped"])
def test_ring_replay(layout, d, dtype):
    """W = 3 causal, 164 rows per rank (ragged against 128 and 256), against
    the reference of the whole sequence."""
    W, cap = 3, 1.5
    shape = (1, W * 164, W * 164, 4, 2, True)
    q, k, v, do = (t.cuda() for t in _inputs(shape, d, dtype))
    got = rr.replay_ring(_Capped(_P(), cap), q, k, v, do, W,
                         1.0 / math.sqrt(d), True, layout, True)
    _check(dict(zip(("o", "lse", "dq", "dk", "dv"), got)),
           _ref(shape, d, dtype, cap), shape, dtype)


# ---- 4. routing and errors ----------------------------------------------------

def test_softcap_zero_is_the_plain_call_bitwise():
    p, d, dtype = _P(), 128, torch.float16
    q, k, v, do = (t.cuda() for t in _inputs(CAUSAL, d, dtype))
    scale = 1.0 / math.sqrt(d)
    o, lse = p.fwd(q, k, v, scale, True)
    o0, lse0 = p.fwd(q, k, v, scale, True, softcap=0.0)
    delta = p.bwd_preprocess(o.to(dtype), do)
    g = p.bwd(do, q, k, v, delta, lse, scale, True, True)
    g0 = p.bwd(do, q, k, v, delta, lse, scale, True, True, softcap=0.0)
    for a, b2 in zip((o, lse, *g), (o0, lse0, *g0)):
        assert torch.equal(a, b2)


def test_backward_bitwise_deterministic():
    a = _fwd_bwd(_P(), CAUSAL, 128, torch.float16, 1.5)
    b2 = _fwd_bwd(_P(), CAUSAL, 128, torch.float16, 1.5)
    for name in a:
        assert torch.equal(a[name], b2[name]), name


@pytest.mark.parametrize("d", [128, 256])
@pytest.mark.parametrize("how,cap,rc,names", [
    ("negative", -1.0, 1008, ("softcap",)),
    ("BA_FWD_SUBT", 1.5, 1002, ("BA_FWD_SUBT", "softcap")),
    ("BA_BWD_FUSED", 1.5, 1002, ("BA_BWD_FUSED", "softcap")),
])
def test_refusals_launch_nothing(how, cap, rc, names, d, monkeypatch):
    """A negative cap, and a cap under a knob that has no cap form: the error
    code, a message naming what was asked, sentinel-filled outputs untouched."""
    from burst_attn_amd._ext import load_extension

    ext, dtype, scale = load_extension(), torch.float16, 1.0 / math.sqrt(d)
    shape = (1, 96, 320, 2, 2, False)
    q, k, v, do = (t.cuda() for t in _inputs(shape, d, dtype))
    f32 = dict(dtype=torch.float32, device="cuda")
    acc = torch.full((1, 96, 2, d), SENTINEL, **f32)
    m, l = (torch.full((1, 2, 96), SENTINEL, **f32) for _ in range(2))
    dq = torch.full((1, 96, 2, d), SENTINEL, **f32)
    dk, dv = (torch.full((1, 320, 2, d), SENTINEL, **f32) for _ in range(2))
    if how != "negative":
        monkeypatch.setenv(how, "0" if how == "BA_FWD_SUBT" else "1")
    calls = []
    if how != "BA_BWD_FUSED":
        calls.append(lambda: ext.attn_fwd_accum(
            q, k, v, scale, False, acc, m, l, False, softcap=cap))
    if how != "BA_FWD_SUBT":
        calls.append(lambda: ext.attn_bwd_accum(
            do, q, k, v, m, l, scale, False, True, dq, dk, dv, softcap=cap))
    for call in calls:
        with pytest.raises(RuntimeError, match=f"rc={rc}") as e:
            call()
        assert all(nm in str(e.value) for nm in names), str(e.value)
    torch.cuda.synchronize()
    for t in (acc, m, l, dq, dk, dv):
        assert bool((t == SENTINEL).all())


@pytest.mark.parametrize("kw", [
    dict(seg=(torch.zeros(1, 96, dtype=torch.int32),
              torch.zeros(1, 320, dtype=torch.int32))),
    dict(band=(0, 64))], ids=["seg", "band"])
def test_provider_refuses_a_cap_with_seg_or_band(kw):
    q, k, v, _ = (t.cuda() for t in _inputs((1, 96, 320, 2, 2, False), 128,
                                            torch.float16))
    with pytest.raises(RuntimeError, match="not supported together"):
        _P().fwd(q, k, v, 0.1, False, softcap=1.5, **kw)


# ---- 5. the public functions on a single-rank ring -----------------------------

@pytest.mark.parametrize("d,dtype", [(256, torch.float16),
                                     (128, torch.bfloat16)])
@pytest.mark.parametrize("striped", [False, True], ids=["zigzag", "striped"])
def test_public_api_single_rank(striped, d, dtype):
    import os

    import torch.distributed as dist

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29713")
        dist.init_process_group("nccl", rank=0, world_size=1)
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    q, k, v, do = (t.cuda() for t in _inputs(CAUSAL, d, dtype))
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(q, k, v, None, "cuda", True, softcap=1.5)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
    _check(dict(o=o, dq=dq, dk=dk, dv=dv), _ref(CAUSAL, d, dtype, 1.5),
           CAUSAL, dtype, ("o", "dq", "dk", "dv"))
