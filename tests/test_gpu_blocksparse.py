"""The HIP kernels with a block mask (block-sparse attention), on one GPU.

Reference: the dense masked softmax of tests/segment_refs.py (``mask=``), the
block mask expanded to an element mask with ``repeat_interleave``, one KV head
at a time (a mask may differ per KV head).  Gates: ``boundary_refs.gates``,
as tests/test_gpu_window.py uses them, gradients under the kernel's own delta.
"""

import functools
import math

import pytest
import torch

from . import segment_refs as sr
from .boundary_inputs import dtype_name as _dt
from .boundary_refs import gates

pytestmark = pytest.mark.gpu

B, SQ, SK = 2, 328, 392
DTYPES = [torch.float16, torch.bfloat16]
_SHAPES = [(d, h, t) for d in (64, 128) for h in ((2, 2), (4, 2))
           for t in DTYPES]
SHAPE = pytest.mark.parametrize(
    "d,heads,dtype", _SHAPES,
    ids=[f"d{d}-n{h[0]}k{h[1]}-{_dt(t)}" for d, h, t in _SHAPES])


def _rand_mask(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) < 0.5).to(torch.uint8)


def _case_mask(name, nk, sq=SQ, sk=SK):
    """(block mask uint8 [Bm, Hm, q blocks, kv blocks], BS)."""
    bs = 128 if name == "bs128" else 64
    nq, nkb = -(-sq // bs), -(-sk // bs)
    if name == "random":
        return _rand_mask((B, nk, nq, nkb), 11), bs
    if name == "bs128":
        return _rand_mask((1, 1, nq, nkb), 12), bs
    m = torch.zeros(1, 1, nq, nkb, dtype=torch.uint8)
    if name == "holes":
        m[..., ::2] = 1
    elif name == "dead":
        m[:] = 1
        m[..., 2, :] = 0
        m[..., :, 3] = 0
    elif name == "one":
        m[..., nq - 1, 2] = 1
    return m, bs


def _elements(m, bs, n_kv, sq, sk):
    """[B, Nk, Sq, Sk] bool of a block mask."""
    e = m.bool().repeat_interleave(bs, 2)[:, :, :sq]
    e = e.repeat_interleave(bs, 3)[:, :, :, :sk]
    return e.expand(B, n_kv, sq, sk)


def _ref(q, k, v, do, scale, emask, o16=None):
    """Dense masked reference, per KV head; with ``o16`` the gradients are
    those under delta = rowsum(o16 * dO), the delta the kernels were given."""
    g = q.shape[2] // k.shape[2]
    outs = []
    for h in range(k.shape[2]):
        qs = slice(h * g, (h + 1) * g)
        a = (q[:, :, qs], k[:, :, h:h + 1], v[:, :, h:h + 1])
        o, lse = sr.seg_fwd(*a, scale, False, None, None, mask=emask[:, h])
        delta = None
        if o16 is not None:
            delta = (o16[:, :, qs] * do[:, :, qs].float()).sum(-1)
            delta = delta.transpose(1, 2).contiguous()
        dq, dk, dv = sr.seg_bwd(do[:, :, qs], *a, lse, scale, False, None, None,
                                delta=delta, o=o, mask=emask[:, h])
        outs.append((o, lse, dq, dk, dv))
    cat = lambda i, dim: torch.cat([t[i] for t in outs], dim)
    return dict(o=cat(0, 2), lse=cat(1, 1), dq=cat(2, 2), dk=cat(3, 2),
                dv=cat(4, 2))


@functools.lru_cache(maxsize=None)
def _inputs(n, nk, d, dtype, sq=SQ, sk=SK):
    g = torch.Generator().manual_seed(77 + n + d)
    r = lambda s, h: torch.randn(B, s, h, d, generator=g).to(dtype)
    return r(sq, n), r(sk, nk), r(sk, nk), r(sq, n)


def _P():
    from burst_attn_amd.tile import HipTileProvider

    return HipTileProvider()


def _run(P, q, k, v, do, scale, causal, blocks):
    kw = {} if blocks is None else {"blocks": blocks}
    o, lse = P.fwd(q, k, v, scale, causal, **kw)
    delta = P.bwd_preprocess(o.to(q.dtype), do)
    dq, dk, dv = P.bwd(do, q, k, v, delta, lse, scale, causal, False, **kw)
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def _assert_gates(got, ref, dtype, g, what):
    gt = gates(dtype, g)
    for name, out in got.items():
        torch.testing.assert_close(
            out.float().cpu(), ref[name], equal_nan=False,
            msg=lambda m, name=name: f"{what} {name}: {m}", **gt[name])


def _check(case, got, emask, dtype, what):
    """Dead rows and unseen keys exactly zero, the rest finite and inside the
    gates."""
    q, k, v, do = case
    g = q.shape[2] // k.shape[2]
    dead = (~emask.any(3)).repeat_interleave(g, 1)      # [B, N, Sq]
    unseen = ~emask.any(2)                              # [B, Nk, Sk]
    o, lse = got["o"].cpu(), got["lse"].cpu()
    assert (o.transpose(1, 2)[dead] == 0).all()
    assert (lse[dead] == -math.inf).all()
    assert (got["dq"].cpu().transpose(1, 2)[dead] == 0).all()
    assert (got["dk"].cpu().transpose(1, 2)[unseen] == 0).all()
    assert (got["dv"].cpu().transpose(1, 2)[unseen] == 0).all()
    for nm in ("o", "dq", "dk", "dv"):
        assert got[nm].isfinite().all(), nm
    assert lse[~dead].isfinite().all()
    scale = 1.0 / math.sqrt(q.shape[3])
    ref = _ref(q, k, v, do, scale, emask, got["o"].to(dtype).float().cpu())
    _assert_gates(got, ref, dtype, g, what)


# 1. tiles against the reference
@SHAPE
@pytest.mark.parametrize("name", ["random", "holes", "dead", "one", "bs128"])
def test_block_tile(name, d, heads, dtype):
    case = _inputs(*heads, d, dtype)
    m, bs = _case_mask(name, heads[1])
    got = _run(_P(), *(t.cuda() for t in case), 1.0 / math.sqrt(d), False,
               (m.cuda(), bs))
    _check(case, got, _elements(m, bs, heads[1], SQ, SK), dtype, f"blk-{name}")


# 2. causal with a mask; a block set above the diagonal changes nothing
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("d,heads", [(128, (4, 2)), (64, (2, 2))])
def test_causal_block_tile(d, heads, dtype):
    case = _inputs(*heads, d, dtype, SQ, SQ)
    m, bs = _case_mask("random", heads[1], SQ, SQ)
    m[..., 1, 4] = 0
    above = m.clone()
    above[..., 1, 4] = 1
    P, dev = _P(), [t.cuda() for t in _inputs(*heads, d, dtype, SQ, SQ)]
    scale = 1.0 / math.sqrt(d)
    got = _run(P, *dev, scale, True, (m.cuda(), bs))
    got2 = _run(P, *dev, scale, True, (above.cuda(), bs))
    for nm in got:
        assert torch.equal(got[nm], got2[nm]), nm
    emask = _elements(m, bs, heads[1], SQ, SQ) & torch.ones(
        SQ, SQ, dtype=torch.bool).tril()
    _check(case, got, emask, dtype, "blk-causal")


# 3. an all-ones mask is the plain call, within the gates
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("causal", [False, True])
def test_all_ones_mask_equals_plain_kernel(causal, dtype):
    dev = [t.cuda() for t in _inputs(4, 2, 128, dtype, SQ, SQ)]
    ones = torch.ones(1, 1, 6, 6, dtype=torch.uint8, device="cuda")
    P, scale = _P(), 1.0 / math.sqrt(128)
    plain = _run(P, *dev, scale, causal, None)
    masked = _run(P, *dev, scale, causal, (ones, 64))
    _assert_gates(masked, {n: t.float().cpu() for n, t in plain.items()}, dtype,
                  2, f"blk-ones-causal{int(causal)}")


# 4. carry-in
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("d,heads", [(128, (4, 2)), (64, (2, 2))])
def test_carry_in_over_key_halves(d, heads, dtype):
    q, k, v, _ = (t.cuda() for t in _inputs(*heads, d, dtype))
    m, bs = _case_mask("random", heads[1])
    m = m.cuda()
    P, scale = _P(), 1.0 / math.sqrt(d)
    o1, lse1 = P.fwd(q, k, v, scale, False, blocks=(m, bs))
    state = P.fwd_accum(None, q, k[:, :192], v[:, :192], scale, False,
                        blocks=(m[..., :3], bs))
    state = P.fwd_accum(state, q, k[:, 192:], v[:, 192:], scale, False,
                        blocks=(m[..., 3:], bs))
    o2, lse2 = P.fwd_finalize(state, dtype)
    gt = gates(dtype, heads[0] // heads[1])
    torch.testing.assert_close(o2.float().cpu(), o1.cpu(), **gt["o"])
    torch.testing.assert_close(lse2.cpu(), lse1.cpu(), **gt["lse"])
    # an all-clear sub-view as the first call: exactly the empty state
    clear = P.fwd_accum(None, q, k, v, scale, False,
                        blocks=(torch.zeros_like(m), bs))
    for x, y in zip(clear, P.fwd_empty_state(q)):
        assert torch.equal(x, y)


# 5. the public API at W = 1
@pytest.mark.parametrize("causal", [True, False])
def test_interface_single_rank_with_block_mask(causal):
    import os

    import torch.distributed as dist

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29713")
        dist.init_process_group("nccl", rank=0, world_size=1)
    from burst_attn_amd import burst_attn_func

    s, bs, d, n, nk = 512, 64, 128, 4, 2
    g = torch.Generator().manual_seed(5)
    r = lambda h: torch.randn(B, s, h, d, generator=g).half()
    q, k, v, do = r(n), r(nk), r(nk), r(n)
    m = _rand_mask((1, nk, s // bs, s // bs), 13)
    m[0, :, 3] = 0  # a dead query block
    emask = _elements(m, bs, nk, s, s)
    if causal:
        emask = emask & torch.ones(s, s, dtype=torch.bool).tril()
    ref = _ref(q, k, v, do, 1.0 / math.sqrt(d), emask)
    qd, kd, vd = (t.cuda().requires_grad_() for t in (q, k, v))
    o = burst_attn_func(qd, kd, vd, None, "cuda", causal,
                        block_mask=m.bool().cuda(), block_size=bs)
    grads = torch.autograd.grad(o, (qd, kd, vd), do.cuda(), retain_graph=True)
    again = torch.autograd.grad(o, (qd, kd, vd), do.cuda())
    for x, y in zip(grads, again):
        assert torch.equal(x, y)
    for nm, out in zip(("o", "dq", "dk", "dv"), (o, *grads)):
        torch.testing.assert_close(out.float().cpu(), ref[nm], rtol=1e-3,
                                   atol=1e-2, msg=lambda t, nm=nm: f"{nm}: {t}")


# 6. refusals leave the outputs untouched
def _refusal(name, mask):
    """(keywords of the extension's accum calls, error pattern, env knob)."""
    ws = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")
    base = {"block_mask": mask, "block_size": 64}
    return {
        "bs48": ({**base, "block_size": 48}, r"rc=1009.*power of two", None),
        "hm3": ({**base, "block_mask": mask.expand(1, 3, -1, -1)},
                r"rc=1009.*Hm=3", None),
        "ws-null": ({**base, "blk_ws": ws(0)}, r"rc=1005.*workspace", None),
        "ws-small": ({**base, "blk_ws": ws(16)}, r"rc=1005.*workspace", None),
        "with-band": ({**base, "band_lo": 0, "band_hi": 40},
                      "not supported together", None),
        "fwd-knob": (base, r"rc=1002.*BA_FWD_SUBT=0.*block mask",
                     ("BA_FWD_SUBT", "0")),
        "bwd-knob": (base, r"rc=1002.*BA_BWD_FUSED=1.*block mask",
                     ("BA_BWD_FUSED", "1")),
        "d256": (base, r"rc=1002.*head_dim 256", None),
    }[name]


@pytest.mark.parametrize("name", ["bs48", "hm3", "ws-null", "ws-small",
                                  "with-band", "fwd-knob", "bwd-knob", "d256"])
def test_refusals_leave_outputs_untouched(name, monkeypatch):
    d = 256 if name == "d256" else 64
    q, k, v, do = (t.cuda() for t in _inputs(2, 2, d, torch.float16))
    sent = lambda *shape: torch.full(shape, 7.0, device="cuda")
    state = (sent(*q.shape), sent(B, 2, SQ), sent(B, 2, SQ))
    dq, dk, dv = sent(*q.shape), sent(*k.shape), sent(*k.shape)
    lse = torch.zeros(B, 2, SQ, device="cuda")
    mask = torch.ones(1, 1, 6, 7, dtype=torch.uint8, device="cuda")
    kw, match, knob = _refusal(name, mask)
    if knob:
        monkeypatch.setenv(*knob)
    ext = _P()._ext
    if name != "bwd-knob":
        with pytest.raises(RuntimeError, match=match):
            ext.attn_fwd_accum(q, k, v, 0.125, False, *state, True, **kw)
    if name != "fwd-knob":
        with pytest.raises(RuntimeError, match=match):
            ext.attn_bwd_accum(do, q, k, v, lse, lse, 0.125, False, False, dq,
                               dk, dv, **kw)
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in (*state, dq, dk, dv))
