"""Block-scaled FP8 forward (descale tensors dq per q row, dk per 64-row kv
tile, dv per v channel) and the HIP quantiser, against plain fp64 attention on
the dequantised inputs.

Tolerance of o (restated from the per-tensor fp8 tests; the scaled form adds
fp32 multiplies only): the 16-bit gate atol 1e-2 + rtol 2e-3 |o| plus the worst
case of rounding P to e4m3, 2^-4 (P @ |V|) for round-to-nearest with three
mantissa bits, plus the flush term (2^-10 / c) sum_j |v_jd|, c = 16 the
kernel's P scale.  The scales of these tests are powers of two, so applying
them is exact and the reference is the kernel's own arithmetic.
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
B, N, NK, D = 2, 4, 2, 128
SCALE = 1.0 / math.sqrt(D)
SHAPES = [(160, 200, False), (200, 200, True), (96, 64, False)]


def _provider():
    from burst_attn_amd.tile import HipTileProvider

    return HipTileProvider()


def _attn64(qd, kd, vd, causal):
    """fp64 o, P @ |V| and sum_j |v_jd| of double q [B,Sq,N,D], k, v."""
    ke, ve = (t.repeat_interleave(qd.shape[2] // t.shape[2], dim=2)
              for t in (kd, vd))
    s = torch.einsum("bqnd,bknd->bnqk", qd, ke) * SCALE
    if causal:
        s = s.masked_fill(~torch.ones(s.shape[-2:], dtype=torch.bool).tril(),
                          -math.inf)
    p = torch.softmax(s, -1)
    return (torch.einsum("bnqk,bknd->bqnd", p, ve),
            torch.einsum("bnqk,bknd->bqnd", p, ve.abs()),
            ve.abs().sum(1, keepdim=True))


def _dequant(q8, k8, v8, dq, dk, dv):
    sk = k8.shape[1]
    return (q8.double() * dq.double().transpose(1, 2)[..., None],
            k8.double() * dk.double().repeat_interleave(64, 2)[:, :, :sk]
            .transpose(1, 2)[..., None],
            v8.double() * dv.double()[:, None])


@functools.lru_cache(maxsize=None)
def _case(sq, sk, causal):
    """fp8 inputs, power-of-two scales that vary by row % 5, tile % 3,
    channel % 4, head and batch, and the fp64 reference, on the CPU."""
    g = torch.Generator().manual_seed(2100 + sq + 3 * sk)
    q8, k8, v8 = (torch.randn(B, s, h, D, generator=g).to(FP8)
                  for s, h in ((sq, N), (sk, NK), (sk, NK)))
    bh = lambda h: (torch.arange(B)[:, None, None]
                    + torch.arange(h)[None, :, None])
    dq = 2.0 ** -(torch.arange(sq) % 5 + bh(N)).float()
    dk = 2.0 ** -(torch.arange(-(-sk // 64)) % 3 + bh(NK) - 1).float()
    dv = 2.0 ** (torch.arange(D) % 4 - bh(NK)).float()
    return (q8, k8, v8, (dq, dk, dv)), _attn64(
        *_dequant(q8, k8, v8, dq, dk, dv), causal)


def _within(o, ref):
    o64, pv, vsum = ref
    bound = 1e-2 + 2e-3 * o64.abs() + 2.0 ** -4 * pv + 2.0 ** -10 / 16 * vsum
    err = (o.double().cpu() - o64).abs()
    print(f"max |err| / bound = {float((err / bound).max()):.3f}")
    return bool((err <= bound).all())


def _cuda(q8, k8, v8, ds):
    return q8.cuda(), k8.cuda(), v8.cuda(), tuple(t.cuda() for t in ds)


def test_constant_scales_equal_float_call():
    (q8, k8, v8, ds), _ = _case(200, 200, True)
    q, k, v, ds = _cuda(q8, k8, v8, ds)
    fl = (0.25, 0.5, 0.125)
    ts = tuple(torch.full_like(t, x) for t, x in zip(ds, fl))
    p = _provider()
    for a, b in zip(p.fwd(q, k, v, SCALE, True, descale=ts),
                    p.fwd(q, k, v, SCALE, True, descale=fl)):
        assert torch.equal(a, b)
    sa, sb = p.fwd_empty_state(q), p.fwd_empty_state(q)
    for _ in range(2):  # the second call carries a non-empty state in
        sa = p.fwd_accum(sa, q, k, v, SCALE, True, descale=ts)
        sb = p.fwd_accum(sb, q, k, v, SCALE, True, descale=fl)
    for a, b in zip(sa, sb):
        assert torch.equal(a, b)


@pytest.mark.parametrize("sq,sk,causal", SHAPES)
def test_indexing(sq, sk, causal):
    (q8, k8, v8, ds), ref = _case(sq, sk, causal)
    q, k, v, ds = _cuda(q8, k8, v8, ds)
    o, _ = _provider().fwd(q, k, v, SCALE, causal, descale=ds)
    assert _within(o, ref)


def test_two_carry_in_rounds():
    """k and v rows [0:128] and [128:200], a dv of its own per round (v is
    re-expressed, exactly, in the second round's units), k_tile0 = 2."""
    (q8, k8, v8, (dq, dk, dv)), _ = _case(160, 200, False)
    v8b = (v8.float() * 2).to(FP8)  # exact: doubling stays far below 448
    vmix = torch.cat([v8[:, :128], v8b[:, 128:]], 1)
    ref = _attn64(*_dequant(q8, k8, v8, dq, dk, dv), False)
    q, k, v, (dq, dk, dv) = _cuda(q8, k8, vmix, (dq, dk, dv))
    p = _provider()
    acc, m, l = p.fwd_empty_state(q)
    for rows, dvr, t0 in ((slice(0, 128), dv, 0), (slice(128, 200), dv / 2, 2)):
        p._ext.attn_fwd_accum(q, k[:, rows], v[:, rows], SCALE, False, acc, m,
                              l, True, descale=(dq, dk, dvr), k_tile0=t0)
    assert _within(acc / l.transpose(1, 2)[..., None], ref)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("mode", ["row", "tile", "channel"])
def test_quantiser(mode, dtype):
    s, h = 200, 3
    g = torch.Generator().manual_seed(77)
    x = (torch.randn(2, s, h, D, generator=g)
         * 2.0 ** torch.randint(-6, 6, (2, s, h, 1), generator=g)).to(dtype)
    x[0, 64:128, 1] = 0  # an all-zero row run, tile and (below) channel
    x[0, :, 1, 5] = 0
    x8, sc = _provider().quantize_fp8(x.cuda(), mode)
    x8, sc, x = x8.cpu().double(), sc.cpu().double(), x.double()
    grp = x.abs().permute(0, 2, 1, 3)  # [B,H,S,D]
    if mode == "row":  # amax per group; spread: a group tensor over x's shape
        amax = grp.amax(3)
        spread = lambda t: t.transpose(1, 2)[..., None]
    elif mode == "tile":
        pad = torch.nn.functional.pad(grp, (0, 0, 0, -s % 64))
        amax = pad.reshape(2, h, -1, 64 * D).amax(3)
        spread = lambda t: t.repeat_interleave(64, 2)[:, :, :s].transpose(
            1, 2)[..., None]
    else:
        amax = grp.amax(2)
        spread = lambda t: t[:, None]
    want = torch.where(amax > 0, amax / 448, torch.ones_like(amax))
    torch.testing.assert_close(sc, want, rtol=1e-6, atol=0)
    assert bool((amax == 0).any()) and bool((sc[amax == 0] == 1.0).all())
    err = (x8 * spread(sc) - x).abs()
    assert bool((err <= 2.0 ** -4 * x.abs() + 2.0 ** -10 * spread(sc)).all())
    top = (x.abs() == spread(amax)) & (x != 0)
    assert bool(top.any()) and bool((x8[top].abs() == 448).all())


def test_outliers_block_scales_beat_per_tensor():
    """One q token, one k tile and one v channel 64 times larger: the error of
    o against fp64 attention on the ORIGINAL values, block scales from the
    quantiser against per-tensor amax / 448 floats."""
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(1, 256, h, D, generator=g).bfloat16()
               for h in (N, NK, NK))
    q[:, 17] *= 64
    k[:, 64:128] *= 64
    v[..., 9] *= 64
    ref = _attn64(q.double(), k.double(), v.double(), True)[0]
    p = _provider()
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    (q8, dq), (k8, dk), (v8, dv) = (p.quantize_fp8(t, mode) for t, mode in (
        (qc, "row"), (kc, "tile"), (vc, "channel")))
    o_blk, _ = p.fwd(q8, k8, v8, SCALE, True, descale=(dq, dk, dv))
    fl = tuple(float(t.abs().max()) / 448 for t in (q, k, v))
    f8 = [(t.float() / s).to(FP8).cuda() for t, s in zip((q, k, v), fl)]
    o_ten, _ = p.fwd(*f8, SCALE, True, descale=fl)
    e_blk, e_ten = (float((o.double().cpu() - ref).abs().mean())
                    for o in (o_blk, o_ten))
    print(f"mean |err| block-scaled {e_blk:.3e}, per-tensor {e_ten:.3e}")
    assert e_blk < e_ten


@pytest.mark.parametrize("striped", [False, True], ids=["zigzag", "striped"])
def test_public_functions_single_rank(striped):
    import os

    import torch.distributed as dist

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29714")
        dist.init_process_group("nccl", rank=0, world_size=1)
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    (q8, k8, v8, ds), ref = _case(256, 256, True)
    q, k, v, ds = _cuda(q8, k8, v8, ds)
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(q, k, v, SCALE, "cuda", True, descale=ds)
    assert o.dtype == torch.bfloat16
    # the bf16 rounding of o, 2^-9 |o|, on top of the kernel's bound
    assert _within(o, (ref[0], ref[1] + 2.0 ** -5 * ref[0].abs(), ref[2]))


@pytest.mark.parametrize("how", ["missing", "dk_short", "dq_shape", "dtype",
                                 "grad", "mixed", "k_off_tile"])
def test_refusals_launch_nothing(how):
    (q8, k8, v8, ds), _ = _case(160, 200, False)
    q, k, v, (dq, dk, dv) = _cuda(q8, k8, v8, ds)
    p = _provider()
    bad = {
        "missing": (dq, dk, None),
        "dk_short": (dq, dk[:, :, :3], dv),
        "dq_shape": (dq[:, :, :100], dk, dv),
        "dtype": (dq, dk.double(), dv),
        "grad": (dq, dk, dv.clone().requires_grad_()),
        "mixed": (dq, 1.0, dv),
        "k_off_tile": (dq, dk, dv),
    }[how]
    acc, m, l = (torch.full_like(t, 7.0) for t in p.fwd_empty_state(q))
    with pytest.raises((RuntimeError, TypeError, ValueError), match="descale"):
        if how == "k_off_tile":  # a k view that starts at row 32 of its tensor
            from burst_attn_amd.interface import _dk_tiles

            _dk_tiles(dk, slice(32, 160), 200, "test")
        p._ext.attn_fwd_accum(q, k, v, SCALE, False, acc, m, l, True,
                              descale=bad)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (acc, m, l))
