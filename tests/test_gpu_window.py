"""The HIP kernels with a band (sliding window), on one GPU.

Reference: the dense masked softmax of tests/segment_refs.py under the band
masks of tests/window_refs.py, on edge-needle inputs for which a band one
off at either edge misses every gate (proved on the CPU by
tests/test_window_cpu.py).  Gates: ``boundary_refs.gates``, those of
tests/test_gpu_parity.py.
"""

import math

import pytest
import torch

from . import segment_refs as sr
from . import window_refs as wr
from . import window_ring_rounds as wrr
from .boundary_inputs import dtype_name as _dt
from .boundary_refs import gates

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
HEADS = [(2, 2), (4, 2)]
SHAPE = pytest.mark.parametrize(
    "d,heads,dtype", [(d, h, t) for d in (64, 128) for h in HEADS
                      for t in DTYPES],
    ids=[f"d{d}-n{h[0]}k{h[1]}-{_dt(t)}" for d in (64, 128) for h in HEADS
         for t in DTYPES])
BIG = 1 << 40


def _P():
    from burst_attn_amd.tile import HipTileProvider

    return HipTileProvider()


def _gpu(c, *names):
    return [c[n].cuda() for n in names]


def _run(P, q, k, v, do, scale, causal, band):
    """Stateless forward, then the backward under its own lse and delta."""
    kw = {} if band is None else {"band": band}
    o, lse = P.fwd(q, k, v, scale, causal, **kw)
    delta = P.bwd_preprocess(o.to(q.dtype), do)
    dq, dk, dv = P.bwd(do, q, k, v, delta, lse, scale, causal, False, **kw)
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def _assert_gates(got, ref, dtype, g, what):
    gt = gates(dtype, g)
    for name, out in got.items():
        out = out.float().cpu()
        print(f"GATE {what} {_dt(dtype)} {name} "
              f"{sr.exceeds(out, ref[name], gt[name]):.3f}")
    for name, out in got.items():
        torch.testing.assert_close(
            out.float().cpu(), ref[name], equal_nan=False,
            msg=lambda m, name=name: f"{what} {name}: {m}", **gt[name])


def _ref_with_kernel_delta(c, got):
    """The reference gradients under the delta the backward was given
    (rowsum of o rounded to the input dtype times dO), as every tile test
    of this suite compares."""
    o16 = got["o"].to(c["q"].dtype).float().cpu()
    delta = (o16 * c["do"].float()).sum(-1).transpose(1, 2).contiguous()
    dq, dk, dv = sr.seg_bwd(c["do"], c["q"], c["k"], c["v"], c["lse"],
                            c["scale"], False, None, None, delta=delta,
                            mask=c["mask"])
    return dict(o=c["o"], lse=c["lse"], dq=dq, dk=dk, dv=dv)


# ---- 1. tiles against the reference ----------------------------------------

@SHAPE
@pytest.mark.parametrize("name", sorted(wr.CASES))
def test_band_tile(name, d, heads, dtype):
    """Rows that see nothing: o = 0, lse = -inf, dq = 0, exactly; keys seen
    by nobody: dk = dv = 0, exactly; everything else finite and inside the
    gates."""
    c = wr.band_case(name, *heads, d, dtype)
    q, k, v, do = _gpu(c, "q", "k", "v", "do")
    got = _run(_P(), q, k, v, do, c["scale"], False, c["band"])
    dead = ~c["mask"][0].any(1)
    unseen = ~c["mask"][0].any(0)
    o, lse = got["o"].cpu(), got["lse"].cpu()
    assert (o[:, dead] == 0).all()
    assert (lse[:, :, dead] == -math.inf).all()
    assert (got["dq"].cpu()[:, dead] == 0).all()
    assert (got["dk"].cpu()[:, unseen] == 0).all()
    assert (got["dv"].cpu()[:, unseen] == 0).all()
    for nm in ("o", "dq", "dk", "dv"):
        assert got[nm].isfinite().all(), nm
    assert lse[:, :, ~dead].isfinite().all()
    _assert_gates(got, _ref_with_kernel_delta(c, got), dtype,
                  heads[0] // heads[1], f"band-{name}")


# ---- 2. causal with a band is the band cut at the diagonal ------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("name,d,heads", [("b", 128, (4, 2)),
                                          ("a", 64, (2, 2))])
def test_causal_band_is_the_cut_band_bitwise(name, d, heads, dtype):
    c = wr.band_case(name, *heads, d, dtype)
    lo, hi = c["band"]
    q, k, v, do = _gpu(c, "q", "k", "v", "do")
    P = _P()
    a = _run(P, q, k, v, do, c["scale"], True, (lo - 7, hi))
    b = _run(P, q, k, v, do, c["scale"], False, (max(lo - 7, 0), hi))
    for nm in a:
        assert torch.equal(a[nm], b[nm]), nm


# ---- 3. a band that covers everything is the plain call, within the gates ----

@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("name,causal,band", [
    ("a", False, (-BIG, BIG)), ("b", True, (-3, BIG)), ("c", False, (-319, 95))])
def test_whole_rectangle_band_equals_plain_kernel(name, causal, band, dtype):
    case = wr.CASES[name]
    c = wr.table_case(name, dtype)
    q, k, v, do = _gpu(c, "q", "k", "v", "do")
    P = _P()
    plain = _run(P, q, k, v, do, c["scale"], causal, None)
    banded = _run(P, q, k, v, do, c["scale"], causal, band)
    _assert_gates(banded, {n: t.float().cpu() for n, t in plain.items()},
                  dtype, case.n // case.nk, f"band-whole-{name}")


# ---- 4. the empty state ---------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("d,heads", [(64, (2, 2)), (128, (4, 2))])
def test_empty_state(d, heads, dtype):
    c = wr.band_case("a", *heads, d, dtype)
    q, k, v = _gpu(c, "q", "k", "v")
    P = _P()
    empty = P.fwd_empty_state(q)
    o0, lse0 = P.fwd_finalize(tuple(t.clone() for t in empty), dtype)
    assert (o0 == 0).all() and (lse0 == -math.inf).all()
    for band in (None, c["band"]):
        kw = {} if band is None else {"band": band}
        fresh = P.fwd_accum(None, q, k, v, c["scale"], False, **kw)
        carried = P.fwd_accum(tuple(t.clone() for t in empty), q, k, v,
                              c["scale"], False, **kw)
        for x, y in zip(P.fwd_finalize(fresh, dtype),
                        P.fwd_finalize(carried, dtype)):
            assert torch.equal(x, y), band
    # a sub-window call at row_offset 165 whose first 100 rows see nothing
    # of it: their state keeps its bits, the others move
    before = tuple(t.clone() for t in carried)
    g = torch.Generator().manual_seed(3 + d)
    k2 = torch.randn(c["k"].shape, generator=g).to(dtype).cuda()
    v2 = torch.randn(c["v"].shape, generator=g).to(dtype).cuda()
    state = P.fwd_accum(carried, q[:, 165:], k2, v2, c["scale"], False,
                        row_offset=165, band=(100, 400))
    acc, m, l = state
    acc0, m0, l0 = before
    keep = slice(0, 265)
    assert torch.equal(acc[:, keep], acc0[:, keep])
    assert torch.equal(m[:, :, keep], m0[:, :, keep])
    assert torch.equal(l[:, :, keep], l0[:, :, keep])
    assert not torch.equal(acc[:, 265:], acc0[:, 265:])
    # and the merged rows are right: rows 265.. see k2[0 .. i - 265]
    o, lse = P.fwd_finalize(state, dtype)
    m1 = wr.band_mask(wr.B, 328, 328, *c["band"])
    m2 = torch.zeros_like(m1)
    m2[:, 165:] = wr.band_mask(wr.B, 163, 328, 100, 400)
    o_ref, lse_ref = sr.seg_fwd(c["q"], torch.cat([c["k"], k2.cpu()], 1),
                                torch.cat([c["v"], v2.cpu()], 1), c["scale"],
                                False, None, None, mask=torch.cat([m1, m2], 2))
    gt = gates(dtype, heads[0] // heads[1])
    torch.testing.assert_close(o.float().cpu(), o_ref, **gt["o"])
    torch.testing.assert_close(lse.cpu(), lse_ref, **gt["lse"])


# ---- 5. ring replay ---------------------------------------------------------------

@pytest.mark.parametrize("d,dtype", [(128, torch.float16),
                                     (64, torch.bfloat16)],
                         ids=["d128-fp16", "d64-bf16"])
@pytest.mark.parametrize("window,causal", [
    ((100, 0), True), ((165, 0), True), ((400, 0), True), ((60, 60), False)],
    ids=["w100", "w165", "w400", "w60x60"])
@pytest.mark.parametrize("W", [3, 4])
def test_ring_replay(W, window, causal, d, dtype):
    c = wrr.ring_case(W, window, causal, d, dtype)
    q, k, v, do = _gpu(c, "q", "k", "v", "do")
    P = _P()
    for layout in ("zigzag", "contiguous", "striped"):
        got = wrr.replay_window_ring(P, q, k, v, do, W, c["scale"], causal,
                                     layout, window)
        got = dict(zip(("o", "lse", "dq", "dk", "dv"), got))
        # the ring's delta is rowsum(o in the input dtype * dO) over whole
        # rows, so the reference gradients follow each replay's own o
        _assert_gates(got, _ref_with_kernel_delta(c, got), dtype,
                      wrr.N // wrr.NK, f"win-ring-{layout}-W{W}-{window}-d{d}")


# ---- 6. errors --------------------------------------------------------------------

def _err_setup():
    c = wr.band_case("d", 2, 2, 64, torch.float16)
    q, k, v, do = _gpu(c, "q", "k", "v", "do")
    lse, delta = c["lse"].cuda(), torch.zeros_like(c["lse"]).cuda()
    sent = lambda t: torch.full(t.shape, 7.0, device="cuda")
    return c, q, k, v, do, lse, delta, sent(q), sent(k), sent(k)


def test_lo_above_hi_is_an_error():
    c, q, k, v, do, lse, delta, dq, dk, dv = _err_setup()
    P = _P()
    with pytest.raises(RuntimeError, match=r"rc=1007.*band"):
        P.fwd(q, k, v, c["scale"], False, band=(5, 4))
    with pytest.raises(RuntimeError, match=r"rc=1007.*band"):
        P.bwd_accum(do, q, k, v, delta, lse, c["scale"], False, False, dq, dk,
                    dv, band=(5, 4))
    torch.cuda.synchronize()
    assert (dq == 7).all() and (dk == 7).all() and (dv == 7).all()


@pytest.mark.parametrize("knob,value,which", [
    ("BA_FWD_SUBT", "0", "fwd"), ("BA_BWD_FUSED", "1", "bwd")])
def test_unsupported_knobs_raise_with_a_band(monkeypatch, knob, value, which):
    c, q, k, v, do, lse, delta, dq, dk, dv = _err_setup()
    P = _P()
    state = (torch.full(q.shape, 7.0, device="cuda"),
             torch.full(lse.shape, 7.0, device="cuda"),
             torch.full(lse.shape, 7.0, device="cuda"))
    monkeypatch.setenv(knob, value)
    with pytest.raises(RuntimeError, match=f"rc=1002.*{knob}={value}.*band"):
        if which == "fwd":
            P.fwd_accum(state, q, k, v, c["scale"], False, band=(0, 40))
        else:
            P.bwd_accum(do, q, k, v, delta, lse, c["scale"], False, False, dq,
                        dk, dv, band=(0, 40))
    torch.cuda.synchronize()
    assert (dq == 7).all() and (dk == 7).all() and (dv == 7).all()
    assert all((t == 7).all() for t in state)


def test_band_with_segment_ids_is_refused():
    c, q, k, v, *_ = _err_setup()
    qs = torch.zeros(q.shape[:2], dtype=torch.int32, device="cuda")
    ks = torch.zeros(k.shape[:2], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="not supported together"):
        _P().fwd(q, k, v, c["scale"], False, seg=(qs, ks), band=(0, 40))


def test_one_band_bound_alone_is_refused():
    c, q, k, v, *_ = _err_setup()
    from burst_attn_amd import _ext

    with pytest.raises(RuntimeError, match="together"):
        _ext.load_extension().attn_fwd(q, k, v, c["scale"], False, band_lo=0)


# ---- 7. the public API at W = 1 -------------------------------------------------------

@pytest.mark.parametrize("striped,causal,window", [
    (False, True, (100, 0)), (True, True, (100, 0)), (False, False, (70, 40))])
def test_interface_single_rank_with_window(striped, causal, window):
    import os

    import torch.distributed as dist

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29713")
        dist.init_process_group("nccl", rank=0, world_size=1)
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    dtype = torch.float16
    name = "a" if causal else "b"
    c = wr.band_case(name, 4, 2, 128, dtype)
    assert c["band"] == (-(0 if causal else window[1]), window[0])
    q, k, v = (c[n].cuda().requires_grad_() for n in ("q", "k", "v"))
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(q, k, v, None, "cuda", causal, window_size=window)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), c["do"].cuda())
    got = {"o": o, "dq": dq, "dk": dk, "dv": dv}
    ref = _ref_with_kernel_delta(c, got)
    gt = gates(dtype, 2)
    for nm, out in got.items():
        torch.testing.assert_close(out.float().cpu(), ref[nm], **gt[nm])
