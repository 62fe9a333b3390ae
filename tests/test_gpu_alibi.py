"""ALiBi: the ALiBi form of the tile kernels against plain fp64 attention with
the one line ``s -= slope[b, h] * |stride * (i - j) + offset|`` added
(tests/alibi_cpu_provider.py), gradients by autograd, cached per case.  Gates:
``boundary_refs.gates`` (TOL, BWD_TOL, LSE_TOL of tests/test_gpu_parity.py),
unchanged.  328 = 256 + 64 + 8 rows put a seam on the 32-row wave, the 64-row
tile, the 256-row block and a ragged tail.  Slopes differ per query head, so
the (4, 2) head cases fail if dK/dV takes one slope per KV head.
"""

import functools
import math

import pytest
import torch

from .alibi_cpu_provider import alibi_attention, std_slopes as _slopes
from .boundary_refs import gates

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16],
                                 ids=lambda t: str(t).split(".")[-1])
# (b, sq, sk, n, nk, causal, offset, stride)
CAUSAL = (1, 328, 328, 4, 2, True, 0, 1)
FULL = (1, 328, 328, 4, 2, False, 0, 1)
SENTINEL = 7.5
NAMES = ("o", "lse", "dq", "dk", "dv")


def _P():
    from burst_attn_amd.tile import HipTileProvider

    return HipTileProvider()


@functools.lru_cache(maxsize=None)
def _inputs(b, sq, sk, n, nk, d, dtype):
    g = torch.Generator().manual_seed(4100 + d + sq + 7 * sk + n)
    return tuple(torch.randn(b, s_, h, d, generator=g).to(dtype)
                 for s_, h in ((sq, n), (sk, nk), (sk, nk), (sq, n)))


@functools.lru_cache(maxsize=None)
def _ref(shape, d, dtype):
    """(o, lse [B,N,S], dq, dk, dv) of ALiBi attention in fp64."""
    b, sq, sk, n, nk, causal, off, stride = shape
    q, k, v, do = (t.double() for t in _inputs(b, sq, sk, n, nk, d, dtype))
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    o, lse = alibi_attention(q, k, v, 1.0 / math.sqrt(d), causal,
                             _slopes(b, n), off, stride)
    grads = torch.autograd.grad(o, (q, k, v), do)
    return {nm: t.detach().float() for nm, t in zip(NAMES, (o, lse, *grads))}


def _check(got, ref, g, dtype, names=NAMES, sel=lambda t, name: t):
    for name in names:
        torch.testing.assert_close(
            got[name].float().cpu(), sel(ref[name], name), **gates(dtype, g)[name],
            msg=lambda m, name=name: f"{name}: {m}")


def _fwd_bwd(p, shape, d, dtype, slopes="ref"):
    b, sq, sk, n, nk, causal, off, stride = shape
    q, k, v, do = (t.cuda() for t in _inputs(b, sq, sk, n, nk, d, dtype))
    sl = _slopes(b, n) if isinstance(slopes, str) else slopes
    kw = {} if sl is None else {"alibi": (sl.cuda(), off, stride)}
    scale = 1.0 / math.sqrt(d)
    o, lse = p.fwd(q, k, v, scale, causal, **kw)
    delta = p.bwd_preprocess(o.to(dtype), do)
    grads = p.bwd(do, q, k, v, delta, lse, scale, causal, True, **kw)
    return dict(zip(NAMES, (o, lse, *grads)))


@DTYPES
@pytest.mark.parametrize("heads", [(2, 2), (4, 2)], ids=str)
@pytest.mark.parametrize("b,sq,sk,causal,off,stride", [
    (1, 328, 328, True, 0, 1), (2, 328, 328, False, 0, 1),
    (1, 96, 320, False, -117, 1), (1, 328, 328, True, 4, 3)], ids=str)
@pytest.mark.parametrize("d", [64, 128])
def test_tile_fwd_bwd(d, b, sq, sk, causal, off, stride, heads, dtype):
    shape = (b, sq, sk, *heads, causal, off, stride)
    _check(_fwd_bwd(_P(), shape, d, dtype), _ref(shape, d, dtype),
           heads[0] // heads[1], dtype)


@DTYPES
def test_carry_in_two_rounds(dtype):
    """Two rounds over the halves of the keys, the second with its offset
    shifted by the split, then finalize, against the joint reference; started
    from fwd_empty_state the same, bit for bit."""
    p, h, d = _P(), 168, 128
    q, k, v, _ = (t.cuda() for t in _inputs(1, 328, 328, 4, 2, d, dtype))
    sl, scale = _slopes(1, 4).cuda(), 1.0 / math.sqrt(d)
    st, st0 = None, p.fwd_empty_state(q)
    for rows, off in ((slice(None, h), 0), (slice(h, None), -h)):
        st, st0 = (p.fwd_accum(s, q, k[:, rows], v[:, rows], scale, False,
                               alibi=(sl, off, 1)) for s in (st, st0))
    o, lse = p.fwd_finalize(st, dtype)
    _check(dict(o=o, lse=lse), _ref(FULL, d, dtype), 2, dtype, ("o", "lse"))
    assert all(torch.equal(a, b2) for a, b2 in zip(st, st0))


@pytest.mark.parametrize("layout,dtype", [("zigzag", torch.float16),
                                          ("striped", torch.bfloat16)])
def test_ring_rounds(layout, dtype):
    """W = 3 causal, 164 rows per rank: the real provider looped over
    ``alibi_tiles`` for every (a, b), against the whole-sequence reference."""
    from burst_attn_amd.interface import alibi_tiles
    from oracle.partition import get_chunk

    p, W, s, d, n, nk = _P(), 3, 164, 128, 4, 2
    scale, sl = 1.0 / math.sqrt(d), _slopes(1, n).cuda()
    ch = lambda t, r, dim=1: get_chunk(t, dim, r, W, zigzag=layout == "zigzag",
                                       striped=layout == "striped")
    full = _inputs(1, W * s, W * s, n, nk, d, dtype)
    q, k, v, do = ([ch(t, r).cuda() for r in range(W)] for t in full)
    f32 = dict(dtype=torch.float32, device="cuda")
    dk, dv = ([torch.zeros(1, s, nk, d, **f32) for _ in range(W)]
              for _ in range(2))
    got = []
    for a in range(W):
        st, dq = p.fwd_empty_state(q[a]), torch.zeros(1, s, n, d, **f32)
        tiles = [(b, t) for b in range(W)
                 for t in alibi_tiles(layout, a, b, W, s, True)]
        for b, (qr, kr, off, stride, tc) in tiles:
            st = p.fwd_accum(st, q[a][:, qr], k[b][:, kr], v[b][:, kr], scale,
                             tc, row_offset=qr.start, alibi=(sl, off, stride))
        o, lse = p.fwd_finalize(st, dtype)
        delta = p.bwd_preprocess(o, do[a])
        for b, (qr, kr, off, stride, tc) in tiles:
            p.bwd_accum(do[a][:, qr], q[a][:, qr], k[b][:, kr], v[b][:, kr],
                        delta[:, :, qr], lse[:, :, qr], scale, tc, True,
                        dq[:, qr], dk[b][:, kr], dv[b][:, kr],
                        alibi=(sl, off, stride))
        got.append(dict(o=o, lse=lse, dq=dq, dk=dk[a], dv=dv[a]))
    ref = _ref((1, W * s, W * s, n, nk, True, 0, 1), d, dtype)
    for a in range(W):  # dk / dv are complete only after every a
        _check(got[a], ref, n // nk, dtype,
               sel=lambda t, name: ch(t, a, 2 if name == "lse" else 1))


def test_routing():
    """Zero slopes equal the plain call within the gates, ``alibi=None`` is the
    plain call bit for bit, and the ALiBi backward is bitwise repeatable."""
    d, dtype = 128, torch.float16
    plain = _fwd_bwd(_P(), CAUSAL, d, dtype, slopes=None)
    zero = _fwd_bwd(_P(), CAUSAL, d, dtype, slopes=torch.zeros(1, 4))
    _check(zero, {k: t.float().cpu() for k, t in plain.items()}, 2, dtype)
    q, k, v, do = (t.cuda() for t in _inputs(1, 328, 328, 4, 2, d, dtype))
    o, lse = _P().fwd(q, k, v, 1.0 / math.sqrt(d), True, alibi=None)
    g = _P().bwd(do, q, k, v, _P().bwd_preprocess(o.to(dtype), do), lse,
                 1.0 / math.sqrt(d), True, True, alibi=None)
    assert all(torch.equal(x, plain[name])
               for x, name in zip((o, lse, *g), NAMES))
    a, b2 = (_fwd_bwd(_P(), CAUSAL, d, dtype) for _ in range(2))
    assert all(torch.equal(a[name], b2[name]) for name in a)


@pytest.mark.parametrize("how,d,stride,rc,names", [
    ("stride", 128, 0, 1011, ("pos_stride",)),
    ("BA_FWD_SUBT", 128, 1, 1002, ("BA_FWD_SUBT", "ALiBi")),
    ("BA_BWD_FUSED", 128, 1, 1002, ("BA_BWD_FUSED", "ALiBi")),
    ("d256", 256, 1, 1002, ("head_dim 256", "ALiBi")),
])
def test_refusals_launch_nothing(how, d, stride, rc, names, monkeypatch):
    """The error code, a message naming what was asked, sentinel-filled
    outputs untouched."""
    from burst_attn_amd._ext import load_extension

    ext, dtype, scale = load_extension(), torch.float16, 1.0 / math.sqrt(d)
    q, k, v, do = (t.cuda() for t in _inputs(1, 96, 320, 2, 2, d, dtype))
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32,
                                     device="cuda")
    acc, dq, m, l = full(1, 96, 2, d), full(1, 96, 2, d), full(1, 2, 96), \
        full(1, 2, 96)
    dk, dv = full(1, 320, 2, d), full(1, 320, 2, d)
    if how.startswith("BA_"):
        monkeypatch.setenv(how, "0" if how == "BA_FWD_SUBT" else "1")
    kw = dict(alibi_slopes=_slopes(1, 2).cuda(), alibi_offset=0,
              alibi_stride=stride)
    calls = []
    if how != "BA_BWD_FUSED":
        calls.append(lambda: ext.attn_fwd_accum(
            q, k, v, scale, False, acc, m, l, False, **kw))
    if how != "BA_FWD_SUBT":
        calls.append(lambda: ext.attn_bwd_accum(
            do, q, k, v, m, l, scale, False, True, dq, dk, dv, **kw))
    for call in calls:
        with pytest.raises(RuntimeError, match=f"rc={rc}") as e:
            call()
        assert all(nm in str(e.value) for nm in names), str(e.value)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (acc, m, l, dq, dk, dv))


def test_public_api_single_rank():
    import os

    import torch.distributed as dist

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29714")
        dist.init_process_group("nccl", rank=0, world_size=1)
    from burst_attn_amd import burst_attn_func

    d, dtype, n, nk = 128, torch.bfloat16, 4, 2
    q, k, v, do = (t.cuda() for t in _inputs(1, 512, 512, n, nk, d, dtype))
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    o = burst_attn_func(q, k, v, None, "cuda", True,
                        alibi_slopes=_slopes(1, n)[0].cuda())
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
    _check(dict(o=o, dq=dq, dk=dk, dv=dv),
           _ref((1, 512, 512, n, nk, True, 0, 1), d, dtype), n // nk, dtype,
           ("o", "dq", "dk", "dv"))
