"""head_dim 256: the one-wave-per-SIMD kernel set against plain fp64 attention.

Reference: softmax(q k^T scale + mask) v and autograd through it, in fp64 on
the CPU, computed once per (shape, dtype) and shared.  Gates: TOL, BWD_TOL
and LSE_TOL of tests/test_gpu_parity.py, unchanged (dk/dv at G x atol, the
rule of tests/test_gpu_gqa.py for a sum of G per-head terms).

Inputs: ``seam_weighted`` / ``diag_needle`` of tests/boundary_inputs.py.
``seam_weighted`` places its hot keys and rows for 256-row workgroups; the
D=256 kernels own 128 rows per workgroup, so keys and rows 127 / 128 get the
same treatment here.  The shapes put a seam on every boundary of the new
kernels: the 32-row wave and backward tile, the forward's 64-row kv tile,
the 128-row block, and the ragged tail (328 = 2 x 128 + 64 + 8).
"""

import functools
import math

import pytest
import torch

from . import boundary_inputs as bi
from .test_gpu_parity import BWD_TOL, LSE_TOL, TOL

pytestmark = pytest.mark.gpu

D = 256
SCALE = 1.0 / math.sqrt(D)
BY_DTYPE = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16],
                                   ids=bi.dtype_name)
# (b, sq, sk, n, nk, causal)
TILES = [
    (1, 328, 328, 4, 4, True), (1, 328, 328, 4, 2, True),
    (2, 328, 328, 4, 2, False), (1, 328, 328, 4, 4, False),
    (1, 96, 320, 4, 2, False), (1, 296, 40, 4, 4, False),
]
BLOCK_SEAMS = (127, 128)


def _ext():
    from burst_attn_amd._ext import load_extension

    return load_extension()


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype, family="seam"):
    b, sq, sk, n, nk, _ = shape
    if family == "needle":
        return bi.diag_needle(b, sq, n, nk, D, dtype, 2560)
    if family == "randn":
        g = torch.Generator().manual_seed(2562)
        return tuple(torch.randn(b, s_, h, D, generator=g).to(dtype)
                     for s_, h in ((sq, n), (sk, nk), (sk, nk), (sq, n)))
    q, k, v, do = bi.seam_weighted(b, sq, sk, n, nk, D, torch.float32, 2561)
    u = bi.seam_vector(D)
    k[:, [j for j in BLOCK_SEAMS if j < sk]] += (
        math.log(max(sk, 2)) / math.sqrt(D)) * u
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
@pytest.mark.parametrize("shape", TILES, ids=str)
def test_tile_fwd_bwd(shape, dtype):
    ref = _ref(shape, dtype)
    o, lse, grads = _fwd_bwd(shape, dtype)
    _close("o", o, ref[0], TOL[dtype])
    _close("lse", lse, ref[1], LSE_TOL)
    _check_grads(shape, dtype, grads, ref)


@BY_DTYPE
def test_diag_needle_causal(dtype):
    """A key one above the diagonal would swamp its row if it leaked through
    the mask, at a 128-row block edge as anywhere."""
    shape = (1, 328, 328, 4, 2, True)
    ref = _ref(shape, dtype, "needle")
    o, lse, grads = _fwd_bwd(shape, dtype, "needle")
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
    st0 = p.fwd_empty_state(q)
    for sl in (slice(None, h), slice(h, None)):
        st0 = p.fwd_accum(st0, q, k[:, sl], v[:, sl], SCALE, False)
    for a, b2 in zip(st, st0):
        assert torch.equal(a, b2)


@BY_DTYPE
def test_strided_views_in_poisoned_parents(dtype):
    """Inputs as strided views into poison, outputs as views into
    sentinel-filled parents: results inside the gates, nothing outside the
    views written."""
    ext = _ext()
    shape = (2, 328, 328, 4, 2, True)
    ref = _ref(shape, dtype)
    pp = bi.poisoned_parent(*_inputs(shape, dtype))
    par = {n_: t.cuda() for n_, t in pp.parents.items()}
    q, k, v, do = (bi.view_of(par[n_], pp.views[n_], pp.parents[n_])
                   for n_ in ("q", "k", "v", "do"))
    outp = {n_: t.cuda() for n_, t in pp.out_parents.items()}
    ov = {n_: bi.view_of(outp[n_], pp.out_views[n_], pp.out_parents[n_])
          for n_ in outp}
    ext.attn_fwd_accum(q, k, v, SCALE, True, ov["acc"], ov["m"], ov["l"],
                       False)
    acc, m, l = (ov[n_].contiguous() for n_ in ("acc", "m", "l"))
    o, lse = ext.attn_fwd_finalize(acc, m, l, dtype)
    _close("o", o, ref[0], TOL[dtype])
    _close("lse", lse, ref[1], LSE_TOL)
    delta = ext.attn_bwd_preprocess(o, do)
    for n_ in ("dq", "dk", "dv"):
        ov[n_].zero_()
    ext.attn_bwd_accum(do, q, k, v, delta, lse, SCALE, True, True, ov["dq"],
                       ov["dk"], ov["dv"])
    _check_grads(shape, dtype, [ov[n_] for n_ in ("dq", "dk", "dv")], ref)
    for n_, parent in outp.items():
        inside = torch.zeros_like(parent, dtype=torch.bool)
        bi.view_of(inside, pp.out_views[n_], pp.out_parents[n_]).fill_(True)
        assert bool((parent[~inside] == bi.SENTINEL).all()), n_


def test_backward_bitwise_deterministic():
    shape, dtype = (1, 328, 328, 4, 2, True), torch.float16
    a, b2 = _fwd_bwd(shape, dtype)[2], _fwd_bwd(shape, dtype)[2]
    for x, y in zip(a, b2):
        assert torch.equal(x, y)


@BY_DTYPE
def test_end_to_end_single_rank(dtype):
    """burst_attn_func on a single-rank ring, causal with optimize_bwd_comm,
    grouped heads, against fp64 attention."""
    import os

    import torch.distributed as dist

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29712")
        dist.init_process_group("nccl", rank=0, world_size=1)
    from burst_attn_amd import burst_attn_func

    shape = (1, 512, 512, 4, 2, True)
    ref = _ref(shape, dtype, "randn")
    q, k, v, do = (t.cuda() for t in _inputs(shape, dtype, "randn"))
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    o = burst_attn_func(q, k, v, None, "cuda", True, True)
    grads = torch.autograd.grad(o, (q, k, v), do)
    if dtype == torch.float16:
        # the reference project's own end-to-end tolerance, o and grads
        tol = dict(rtol=1e-3, atol=1e-2)
        for name, out, r in zip(("o", "dq", "dk", "dv"), (o, *grads),
                                (ref[0], *ref[2:])):
            _close(name, out, r, tol)
    else:  # the bf16 row of test_interface_flags_single_rank
        _close("o", o, ref[0], TOL[dtype])
        _check_grads(shape, dtype, grads, ref)


@pytest.mark.parametrize("how", ["seg", "band", "BA_FWD_SUBT", "BA_BWD_FUSED"])
def test_refusals(how, monkeypatch):
    """What D=256 does not serve raises an error naming it; the next plain
    call succeeds."""
    from burst_attn_amd.tile import HipTileProvider

    shape, dtype, p = (1, 96, 320, 4, 4, False), torch.float16, HipTileProvider()
    q, k, v, do = (t.cuda() for t in _inputs(shape, dtype))
    o, lse = p.fwd(q, k, v, SCALE, False)
    delta = p.bwd_preprocess(o.to(dtype), do)
    ids = (torch.zeros(1, 96, dtype=torch.int32, device="cuda"),
           torch.zeros(1, 320, dtype=torch.int32, device="cuda"))
    if how == "seg":
        call, names = (lambda: p.fwd(q, k, v, SCALE, False, seg=ids)), "segment"
    elif how == "band":
        call, names = (lambda: p.fwd(q, k, v, SCALE, False, band=(0, 64))), "band"
    elif how == "BA_FWD_SUBT":
        monkeypatch.setenv(how, "2")
        call, names = (lambda: p.fwd(q, k, v, SCALE, False)), how
    else:
        monkeypatch.setenv(how, "1")
        call, names = (lambda: p.bwd(do, q, k, v, delta, lse, SCALE, False,
                                     True)), how
    with pytest.raises(RuntimeError, match=names) as e:
        call()
    assert "256" in str(e.value)
    monkeypatch.delenv(how, raising=False)
    o2, _ = p.fwd(q, k, v, SCALE, False)
    assert torch.equal(o, o2)
