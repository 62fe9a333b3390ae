"""q/k head_dim 192 with v head_dim 128: the kernel set against plain fp64
attention.

Reference: softmax(q k^T / sqrt(192) + mask) v and autograd through it, in
fp64 on the CPU, computed once per (shape, dtype) and shared.  Gates: TOL,
BWD_TOL and LSE_TOL of tests/test_gpu_parity.py, unchanged (dk/dv at G x
atol, the rule of tests/test_gpu_gqa.py for a sum of G per-head terms).

Inputs: ``seam_weighted`` / ``diag_needle`` of tests/boundary_inputs.py, q and
k from the 192-wide call, v and dO from the 128-wide call.  The kernels own
128 rows per workgroup, so keys and rows 127 / 128 get the hot-key and dO
treatment too (as in tests/test_gpu_d256.py).  The shapes put a seam on every
boundary of the split: the 32-row wave and backward tile, the forward's
64-row kv tile, the 128-row block, and the ragged tail (328 = 2 x 128 + 64 +
8).
"""

import functools
import math

import pytest
import torch

from . import boundary_inputs as bi
from .test_gpu_parity import BWD_TOL, LSE_TOL, TOL

pytestmark = pytest.mark.gpu

DQK, DV = 192, 128
SCALE = 1.0 / math.sqrt(DQK)
BY_DTYPE = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16],
                                   ids=bi.dtype_name)
# (b, sq, sk, n, nk, causal)
TILES = [
    (1, 328, 328, 4, 4, True), (1, 328, 328, 4, 2, True),
    (2, 328, 328, 4, 2, False), (1, 96, 320, 4, 2, False),
    (1, 296, 40, 4, 4, False),
]
BLOCK_SEAMS = (127, 128)


def _ext():
    from burst_attn_amd._ext import load_extension

    return load_extension()


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype, family="seam"):
    b, sq, sk, n, nk, _ = shape
    if family == "needle":
        q, k, _, _ = bi.diag_needle(b, sq, n, nk, DQK, dtype, 1920)
        _, _, v, do = bi.diag_needle(b, sq, n, nk, DV, dtype, 1920)
        return q, k, v, do
    if family == "randn":
        g = torch.Generator().manual_seed(1922)
        return tuple(torch.randn(b, s_, h, d, generator=g).to(dtype)
                     for s_, h, d in ((sq, n, DQK), (sk, nk, DQK),
                                      (sk, nk, DV), (sq, n, DV)))
    q, k, _, _ = bi.seam_weighted(b, sq, sk, n, nk, DQK, torch.float32, 1921)
    _, _, v, do = bi.seam_weighted(b, sq, sk, n, nk, DV, torch.float32, 1921)
    k[:, [j for j in BLOCK_SEAMS if j < sk]] += (
        math.log(max(sk, 2)) / math.sqrt(DQK)) * bi.seam_vector(DQK)
    do[:, [i for i in BLOCK_SEAMS if i < sq]] *= bi.DO_GAIN
    return tuple(t.to(dtype) for t in (q, k, v, do))


@functools.lru_cache(maxsize=None)
def _ref(shape, dtype, family="seam"):
    """(o, lse [B,N,S], dq, dk, dv) of plain attention in fp64."""
    n, nk, causal = shape[3], shape[4], shape[5]
    q, k, v, do = (t.double() for t in _inputs(shape, dtype, family))
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    ke, ve = (t.repeat_interleave(n // nk, dim=2) for t in (k, v))
    s = torch.einsum("bqnd,bknd->bnqk", q, ke) * SCALE
    if causal:
        s = s.masked_fill(~torch.ones(s.shape[-2:], dtype=torch.bool).tril(),
                          -math.inf)
    o = torch.einsum("bnqk,bknd->bqnd", torch.softmax(s, -1), ve)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
    return tuple(t.detach().float()
                 for t in (o, torch.logsumexp(s, -1), dq, dk, dv))


def _close(name, out, ref, gate, atol_x=1):
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    torch.testing.assert_close(
        out.float().cpu(), ref, rtol=gate["rtol"], atol=atol_x * gate["atol"],
        msg=lambda m: f"{name}: {m}")


def _check_grads(shape, dtype, grads, ref):
    g = shape[3] // shape[4]
    for name, out, r, x in zip(("dq", "dk", "dv"), grads, ref[2:], (1, g, g)):
        _close(name, out, r, BWD_TOL[dtype], x)


def _fwd_bwd(shape, dtype, family="seam"):
    ext = _ext()
    q, k, v, do = (t.cuda() for t in _inputs(shape, dtype, family))
    o, lse = ext.attn_fwd(q, k, v, SCALE, shape[5])
    delta = ext.attn_bwd_preprocess(o.to(dtype), do)
    return o, lse, ext.attn_bwd(do, q, k, v, delta, lse, SCALE, shape[5], True)


@BY_DTYPE
@pytest.mark.parametrize("shape,family", [(s, "seam") for s in TILES]
                         + [((1, 328, 328, 4, 2, True), "needle")], ids=str)
def test_tile_fwd_bwd(shape, family, dtype):
    """The seam table, and diag_needle causal at S = 328: a key one above the
    diagonal would swamp its row if it leaked through the mask."""
    ref = _ref(shape, dtype, family)
    o, lse, grads = _fwd_bwd(shape, dtype, family)
    _close("o", o, ref[0], TOL[dtype])
    _close("lse", lse, ref[1], LSE_TOL)
    _check_grads(shape, dtype, grads, ref)


@BY_DTYPE
def test_carry_in_two_rounds(dtype):
    """Two rounds over the halves of the keys, then finalize, against the
    joint reference; started from fwd_empty_state the same, bit for bit."""
    from burst_attn_amd.tile import HipTileProvider

    shape = (1, 328, 328, 4, 2, False)
    ref = _ref(shape, dtype)
    q, k, v, _ = (t.cuda() for t in _inputs(shape, dtype))
    p, h = HipTileProvider(), 168
    st = p.fwd_accum(None, q, k[:, :h], v[:, :h], SCALE, False)
    st = p.fwd_accum(st, q, k[:, h:], v[:, h:], SCALE, False)
    o, lse = p.fwd_finalize(st, dtype)
    _close("o", o, ref[0], TOL[dtype])
    _close("lse", lse, ref[1], LSE_TOL)
    st0 = p.fwd_empty_state(q, DV)
    for sl in (slice(None, h), slice(h, None)):
        st0 = p.fwd_accum(st0, q, k[:, sl], v[:, sl], SCALE, False)
    for a, b2 in zip(st, st0):
        assert torch.equal(a, b2)


def test_bwd_accum_strided_and_deterministic():
    """bwd_accum into strided fp32 views pre-filled with a constant equals
    bwd + constant, and the backward is bitwise run-to-run identical."""
    ext = _ext()
    shape, dtype, c = (1, 328, 328, 4, 2, True), torch.float16, 3.0
    q, k, v, do = (t.cuda() for t in _inputs(shape, dtype))
    o, lse, grads = _fwd_bwd(shape, dtype)
    for x, y in zip(grads, _fwd_bwd(shape, dtype)[2]):
        assert torch.equal(x, y)
    delta = ext.attn_bwd_preprocess(o.to(dtype), do)
    # views: every other row of a parent twice as long, heads 1.. of one more
    views = []
    for g_ in grads:
        b, s, h, d = g_.shape
        parent = torch.full((b, 2 * s, h + 1, d), c, device="cuda")
        views.append(parent[:, ::2, 1:])
    ext.attn_bwd_accum(do, q, k, v, delta, lse, SCALE, True, True, *views)
    for name, view, g_ in zip(("dq", "dk", "dv"), views, grads):
        assert torch.equal(view, g_ + c), name


@pytest.mark.parametrize("striped", [False, True], ids=["zigzag", "striped"])
def test_end_to_end_single_rank(striped):
    """burst_attn_func / burst_attn_func_striped on a single-rank ring with
    autograd, causal with optimize_bwd_comm, grouped heads, default scale, at
    the reference project's own end-to-end tolerance."""
    import os

    import torch.distributed as dist

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29713")
        dist.init_process_group("nccl", rank=0, world_size=1)
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    shape, dtype = (1, 512, 512, 4, 2, True), torch.float16
    ref = _ref(shape, dtype, "randn")
    q, k, v, do = (t.cuda() for t in _inputs(shape, dtype, "randn"))
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(q, k, v, None, "cuda", True, True)
    grads = torch.autograd.grad(o, (q, k, v), do)
    tol = dict(rtol=1e-3, atol=1e-2)
    for name, out, r in zip(("o", "dq", "dk", "dv"), (o, *grads),
                            (ref[0], *ref[2:])):
        _close(name, out, r, tol)


@pytest.mark.parametrize("how", ["192x96", "128x192", "BA_FWD_SUBT",
                                 "BA_BWD_FUSED"])
def test_refusals(how, monkeypatch):
    """Other width pairs raise naming both widths, a knob value at (192, 128)
    raises naming the knob, all before any launch; the next plain call
    succeeds."""
    ext = _ext()
    shape, dtype = (1, 96, 320, 4, 4, False), torch.float16
    q, k, v, do = (t.cuda() for t in _inputs(shape, dtype))
    o, lse = ext.attn_fwd(q, k, v, SCALE, False)
    delta = ext.attn_bwd_preprocess(o.to(dtype), do)
    if how == "192x96":
        call, names = (lambda: ext.attn_fwd(q, k, v[..., :96].contiguous(),
                                            SCALE, False)), ("192", "96")
    elif how == "128x192":
        call, names = (lambda: ext.attn_fwd(
            q[..., :128].contiguous(), k[..., :128].contiguous(), k, SCALE,
            False)), ("128", "192")
    elif how == "BA_FWD_SUBT":
        monkeypatch.setenv(how, "2")
        call, names = (lambda: ext.attn_fwd(q, k, v, SCALE, False)), (how,)
    else:
        monkeypatch.setenv(how, "1")
        call, names = (lambda: ext.attn_bwd(do, q, k, v, delta, lse, SCALE,
                                            False, True)), (how,)
    with pytest.raises(RuntimeError) as e:
        call()
    assert all(n_ in str(e.value) for n_ in names), str(e.value)
    monkeypatch.delenv(how, raising=False)
    o2, _ = ext.attn_fwd(q, k, v, SCALE, False)
    assert torch.equal(o, o2)
