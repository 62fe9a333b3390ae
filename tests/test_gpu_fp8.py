"""FP8 e4m3 forward (K = 64 MFMA kernel set) against plain fp64 attention on
the dequantised inputs (q8.double() * sq and so on), computed once per case.

Exact-P family (the sharp gate): softmax_scale = ln 2, one-hot q rows and k
entries in {0, -1, -2, -3} make every exp2-domain score an integer, so every
P is a power of two, exactly representable in e4m3: FP8 adds no error and the
fp64 reference is the exact answer of the kernel's own arithmetic.  Gates:
TOL[fp16] on o, LSE_TOL on lse, unchanged from tests/test_gpu_parity.py.

Quantised realistic family: seam_weighted / diag_needle scaled to amax / 448.
lse at LSE_TOL (fp8 products are exact in fp32); o within TOL[fp16] plus the
worst case of rounding P: 2^-4 (P @ |V|) for round-to-nearest with three
mantissa bits plus the flush term (2^-10 / c) sum_j |v_jd|, c the kernel's P
scale.  The bound is loose (profiles/fp8/README.md has max |err| / bound).
"""

import functools
import math

import pytest
import torch

from . import boundary_inputs as bi
from .test_gpu_parity import LSE_TOL, TOL

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
D = 128
# (b, sq, sk, n, nk, causal): the tile shapes of tests/test_gpu_d256.py
TILES = [
    (1, 328, 328, 4, 4, True), (1, 328, 328, 4, 2, True),
    (2, 328, 328, 4, 2, False), (1, 96, 320, 4, 2, False),
    (1, 296, 40, 4, 4, False),
]
F16 = TOL[torch.float16]


def _provider():
    from burst_attn_amd.tile import HipTileProvider

    return HipTileProvider()


@functools.lru_cache(maxsize=None)
def _case(shape, family):
    """(q8, k8, v8, descale, scale) on the CPU and the fp64 reference
    (o, lse [B,N,S], P @ |V|, sum_j |v_jd| per kv head)."""
    b, sq, sk, n, nk, causal = shape
    g = torch.Generator().manual_seed(808 + sq + 3 * sk + nk)
    if family == "exact":
        q = torch.zeros(b, sq, n, D).scatter_(
            3, torch.randint(0, D, (b, sq, n, 1), generator=g), 1.0)
        k = -torch.randint(0, 4, (b, sk, nk, D), generator=g).float()
        v = torch.randn(b, sk, nk, D, generator=g)
        q8, k8, v8 = (t.to(FP8) for t in (q, k, v))
        descale, scale = (1.0, 1.0, 0.25), math.log(2.0)
    else:
        if family == "needle":
            q, k, v, _ = bi.diag_needle(b, sq, n, nk, D, torch.float32, 2580)
        else:
            q, k, v, _ = bi.seam_weighted(b, sq, sk, n, nk, D, torch.float32,
                                          2581)
        descale = tuple(float(t.abs().max()) / 448.0 for t in (q, k, v))
        q8, k8, v8 = ((t / s).to(FP8) for t, s in zip((q, k, v), descale))
        scale = 1.0 / math.sqrt(D)
    qd, kd, vd = (t.float().double() * s
                  for t, s in zip((q8, k8, v8), descale))
    ke, ve = (t.repeat_interleave(n // nk, dim=2) for t in (kd, vd))
    s = torch.einsum("bqnd,bknd->bnqk", qd, ke) * scale
    if causal:
        s = s.masked_fill(~torch.ones(sq, sk, dtype=torch.bool).tril(),
                          -math.inf)
    p = torch.softmax(s, -1)
    ref = (torch.einsum("bnqk,bknd->bqnd", p, ve), torch.logsumexp(s, -1),
           torch.einsum("bnqk,bknd->bqnd", p, ve.abs()),
           ve.abs().sum(1, keepdim=True))
    return (q8, k8, v8, descale, scale), tuple(t.float() for t in ref)


def _close(name, out, ref, gate):
    torch.testing.assert_close(out.float().cpu(), ref, rtol=gate["rtol"],
                               atol=gate["atol"], msg=lambda m: f"{name}: {m}")


@pytest.mark.parametrize("shape", TILES, ids=str)
def test_exact_p(shape):
    (q, k, v, ds, scale), ref = _case(shape, "exact")
    o, lse = _provider().fwd(q.cuda(), k.cuda(), v.cuda(), scale, shape[5],
                             descale=ds)
    _close("o", o, ref[0], F16)
    _close("lse", lse, ref[1], LSE_TOL)


@pytest.mark.parametrize("shape,family", [(s, "seam") for s in TILES]
                         + [((1, 328, 328, 4, 2, True), "needle")], ids=str)
def test_quantised_realistic(shape, family):
    (q, k, v, ds, scale), ref = _case(shape, family)
    p = _provider()
    o, lse = p.fwd(q.cuda(), k.cuda(), v.cuda(), scale, shape[5], descale=ds)
    _close("lse", lse, ref[1], LSE_TOL)
    c = p._ext.attn_fp8_p_scale()
    bound = (F16["atol"] + F16["rtol"] * ref[0].abs() + 2.0 ** -4 * ref[2]
             + (2.0 ** -10 / c) * ref[3])
    err = (o.cpu() - ref[0]).abs()
    print(f"fp8 {family} {shape}: max |err| / bound = "
          f"{float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


def test_carry_in_two_rounds():
    """Two rounds over the key halves, then finalize to bf16, against the
    joint reference; started from fwd_empty_state the same, bit for bit."""
    (q, k, v, ds, scale), ref = _case((1, 328, 328, 4, 2, False), "exact")
    q, k, v = q.cuda(), k.cuda(), v.cuda()
    p, h = _provider(), 168
    halves = (slice(None, h), slice(h, None))
    st, st0 = None, p.fwd_empty_state(q)
    for sl in halves:
        st = p.fwd_accum(st, q, k[:, sl], v[:, sl], scale, False, descale=ds)
        st0 = p.fwd_accum(st0, q, k[:, sl], v[:, sl], scale, False, descale=ds)
    o, lse = p.fwd_finalize(st, torch.bfloat16)
    _close("o", o, ref[0], TOL[torch.bfloat16])
    _close("lse", lse, ref[1], LSE_TOL)
    for a, b2 in zip(st, st0):
        assert torch.equal(a, b2)


def test_strided_views_in_poisoned_parents():
    """Causal GQA through strided views into poison, the state as views into
    sentinel-filled parents: inside the gates, nothing outside written."""
    (q, k, v, ds, scale), ref = _case((2, 328, 328, 4, 2, True), "exact")
    pp = bi.poisoned_parent(q.float(), k.float(), v.float(), q.float())
    par = {n_: t.clamp(-448, 448).to(FP8).cuda()
           for n_, t in pp.parents.items()}
    qv, kv, vv = (bi.view_of(par[n_], pp.views[n_], pp.parents[n_])
                  for n_ in ("q", "k", "v"))
    outp = {n_: pp.out_parents[n_].cuda() for n_ in ("acc", "m", "l")}
    ov = {n_: bi.view_of(outp[n_], pp.out_views[n_], pp.out_parents[n_])
          for n_ in outp}
    p = _provider()
    p._ext.attn_fwd_accum(qv, kv, vv, scale, True, ov["acc"], ov["m"],
                          ov["l"], False, descale=ds)
    o, lse = p.fwd_finalize([ov[n_].contiguous() for n_ in ("acc", "m", "l")],
                            torch.float16)
    _close("o", o, ref[0], F16)
    _close("lse", lse, ref[1], LSE_TOL)
    for n_, parent in outp.items():
        inside = torch.zeros_like(parent, dtype=torch.bool)
        bi.view_of(inside, pp.out_views[n_], pp.out_parents[n_]).fill_(True)
        assert bool((parent[~inside] == bi.SENTINEL).all()), n_


@pytest.mark.parametrize("coding", ["index", "ints"])
def test_mfma_k64_layout_probe(coding):
    """One 32x32x64 fp8 MFMA with operands placed as attn_fp8.h states,
    against a host matmul, exact.  "index": one-hot A rows select rows of a B
    whose 64 k rows carry 64 distinct e4m3 values."""
    g = torch.Generator().manual_seed(64)
    if coding == "index":
        a = torch.zeros(32, 64).scatter_(
            1, torch.randint(0, 64, (32, 1), generator=g), 1.0)
        kk = torch.arange(64.0)
        b = (2.0 ** (kk % 8 - 4) * (1 + (kk // 8) / 8))[:, None] * (
            1 - 2 * (torch.arange(32) % 2))[None, :]
    else:
        a = torch.randint(-8, 9, (32, 64), generator=g).float()
        b = torch.randint(-8, 9, (64, 32), generator=g).float()
    d = _provider()._ext.fp8_mfma_probe(a.to(FP8).cuda(), b.to(FP8).cuda())
    assert torch.equal(d.cpu(), a @ b)


def test_end_to_end_single_rank():
    """burst_attn_func on a single-rank ring, causal, s = 512."""
    import os

    import torch.distributed as dist

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29713")
        dist.init_process_group("nccl", rank=0, world_size=1)
    from burst_attn_amd import burst_attn_func

    (q, k, v, ds, scale), ref = _case((1, 512, 512, 4, 2, True), "exact")
    o = burst_attn_func(q.cuda(), k.cuda(), v.cuda(), scale, "cuda", True,
                        descale=ds)
    assert o.dtype == torch.bfloat16
    _close("o", o, ref[0], TOL[torch.bfloat16])


@pytest.mark.parametrize("how", [
    "seg", "band", "softcap", "blocks", "head_dim", "v_width", "v_width_accum",
    "BA_FWD_SUBT", "module", "descale_zero", "descale_nan", "descale_v_tiny",
    "bwd", "descale_fp16"])
def test_refusals(how, monkeypatch):
    """What fp8 does not serve raises an error naming it; the next plain fp16
    call gives the bits it gave before."""
    p = _provider()
    (q, k, v, ds, scale), _ = _case((1, 96, 320, 4, 2, False), "exact")
    qh, kh, vh = (t.half().cuda() for t in (q, k, v))
    q, k, v = q.cuda(), k.cuda(), v.cuda()
    o, lse = p.fwd(qh, kh, vh, scale, False)
    fwd = lambda **kw: p.fwd(q, k, v, scale, False, **kw)
    ids = (torch.zeros(1, 96, dtype=torch.int32, device="cuda"),
           torch.zeros(1, 320, dtype=torch.int32, device="cuda"))
    mask = torch.ones(1, 1, 2, 5, dtype=torch.uint8, device="cuda")

    def module():  # the module kernel, handed fp8 inputs and a full state
        monkeypatch.setenv("BA_FWD_ASM", "1")
        pa = _provider()
        pa._ext.attn_fwd_accum_asm(q, k, v, scale, False,
                                   *pa.fwd_empty_state(q), True)

    call, names = {
        "seg": (lambda: fwd(seg=ids), "fp8.*seg"),
        "band": (lambda: fwd(band=(0, 64)), "fp8.*band"),
        "softcap": (lambda: fwd(softcap=30.0), "fp8.*softcap"),
        "blocks": (lambda: fwd(blocks=(mask, 64)), "fp8.*blocks"),
        "head_dim": (lambda: p.fwd(q[..., :64], k[..., :64], v[..., :64],
                                   scale, False), "fp8.*head_dim 64"),
        "v_width": (lambda: p.fwd(q, k, v[..., :64], scale, False),
                    "fp8.*head_dim, got 128 and 64"),
        "v_width_accum": (lambda: p.fwd_accum(None, q, k, v[..., :64], scale,
                                              False),
                          "fp8.*head_dim, got 128 and 64"),
        "BA_FWD_SUBT": (lambda: fwd(), "BA_FWD_SUBT=2.*fp8"),
        "module": (module, "fp8.*module"),
        "descale_zero": (lambda: fwd(descale=(1.0, 0.0, 1.0)), "descale"),
        "descale_nan": (lambda: fwd(descale=(1.0, 1.0, math.nan)), "descale"),
        "descale_v_tiny": (lambda: fwd(descale=(1.0, 1.0, 1e-45)), "descale"),
        "bwd": (lambda: p.bwd(qh, q, k, v, lse, lse, scale, False, True),
                "fp8"),
        "descale_fp16": (lambda: p.fwd(qh, kh, vh, scale, False, descale=ds),
                         "descale"),
    }[how]
    if how == "BA_FWD_SUBT":
        monkeypatch.setenv(how, "2")
    with pytest.raises(RuntimeError, match=names):
        call()
    monkeypatch.delenv("BA_FWD_SUBT", raising=False)
    o2, _ = p.fwd(qh, kh, vh, scale, False)
    assert torch.equal(o, o2)
