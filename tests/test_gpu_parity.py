"""GPU parity tests: gfx950 HIP kernels vs the CPU oracle.

All marked @pytest.mark.gpu (run via gpurun / the round-end driver on a real
MI355X).  The oracle is computed live on CPU from the same seeded inputs —
nothing here reads /root/reference.

Tolerances: inputs are fp16/bf16, kernel accumulates fp32 (matching the
flash path the reference uses); the reference's own parity gate is
rtol=1e-3, atol=1e-2 at fp16 (test/checker.py:10).  bf16 inputs get a
looser atol (3x fewer mantissa bits).
"""

import math

import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

TOL = {
    torch.float16: dict(rtol=2e-3, atol=1e-2),
    torch.bfloat16: dict(rtol=2e-2, atol=5e-2),
}
BWD_TOL = {
    torch.float16: dict(rtol=5e-3, atol=2e-2),
    torch.bfloat16: dict(rtol=3e-2, atol=1e-1),
}
LSE_TOL = dict(rtol=1e-3, atol=2e-2)


def _ext():
    from burst_attn_amd._ext import load_extension

    return load_extension()


def _rand(b, s, n, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, s, n, d, generator=g).to(dtype).cuda()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_mfma_layout_probe(dtype):
    """Pin the assumed 32x32x16 MFMA A/B/D lane maps with an ASYMMETRIC
    matmul (a symmetric one passes transposed layouts silently)."""
    g = torch.Generator().manual_seed(99)
    a = torch.randn(32, 16, generator=g).to(dtype).cuda()
    b = (torch.randn(16, 32, generator=g) * torch.linspace(0.2, 2.0, 32)).to(dtype).cuda()
    d = _ext().mfma_probe(a, b)
    ref = a.float().cpu() @ b.float().cpu()
    torch.testing.assert_close(d.cpu(), ref, rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize(
    "b,sq,sk,n,d",
    [
        (1, 256, 256, 2, 128),
        (2, 512, 512, 3, 128),
        (1, 256, 256, 2, 64),
        (1, 96, 320, 2, 128),   # uneven, sq != sk (non-causal only)
        (1, 300, 300, 1, 128),  # ragged tails
    ],
)
def test_fwd_tile_parity(b, sq, sk, n, d, causal, dtype):
    if causal and sq != sk:
        pytest.skip("causal tiles are equal-length")
    q = _rand(b, sq, n, d, dtype, 1)
    k = _rand(b, sk, n, d, dtype, 2)
    v = _rand(b, sk, n, d, dtype, 3)
    scale = 1.0 / math.sqrt(d)
    o, lse = _ext().attn_fwd(q, k, v, scale, causal)
    o_ref, lse_ref = oracle.tile_fwd(q.cpu(), k.cpu(), v.cpu(), scale, causal)
    torch.testing.assert_close(o.cpu(), o_ref, **TOL[dtype])
    torch.testing.assert_close(lse.cpu(), lse_ref, **LSE_TOL)


@pytest.mark.parametrize("dtype", [torch.float16])
def test_fwd_strided_slices(dtype):
    """The ring passes sliced views (zigzag halves / striped shifts) —
    exercise non-contiguous seq slices through the stride path."""
    b, s, n, d = 2, 256, 2, 128
    q = _rand(b, s, n, d, dtype, 7)
    k = _rand(b, s, n, d, dtype, 8)
    v = _rand(b, s, n, d, dtype, 9)
    half = s // 2
    scale = 1.0 / math.sqrt(d)
    # q second half vs full kv (zigzag round), via views not copies
    o, lse = _ext().attn_fwd(q[:, half:], k, v, scale, False)
    o_ref, lse_ref = oracle.tile_fwd(q.cpu()[:, half:], k.cpu(), v.cpu(), scale, False)
    torch.testing.assert_close(o.cpu(), o_ref, **TOL[dtype])
    # striped shift: q[1:] vs k[:-1] (odd offsets exercise alignment)...
    # shift by one keeps 16B alignment because N*D is a multiple of 8
    o2, _ = _ext().attn_fwd(q[:, 1:], k[:, :-1], v[:, :-1], scale, True)
    o2_ref, _ = oracle.tile_fwd(q.cpu()[:, 1:], k.cpu()[:, :-1], v.cpu()[:, :-1], scale, True)
    torch.testing.assert_close(o2.cpu(), o2_ref, **TOL[dtype])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_bwd_preprocess(dtype):
    b, s, n, d = 2, 192, 3, 128
    o = _rand(b, s, n, d, dtype, 11)
    do = _rand(b, s, n, d, dtype, 12)
    delta = _ext().attn_bwd_preprocess(o, do)
    ref = (o.float() * do.float()).sum(-1).transpose(1, 2).cpu()
    torch.testing.assert_close(delta.cpu(), ref, rtol=1e-3, atol=1e-2)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize(
    "b,sq,sk,n,d",
    [
        (1, 256, 256, 2, 128),
        (1, 512, 512, 2, 128),
        (1, 256, 256, 2, 64),
        (1, 128, 320, 2, 128),  # sq != sk
        (1, 200, 200, 1, 128),  # ragged
    ],
)
def test_bwd_tile_parity(b, sq, sk, n, d, causal, dtype):
    if causal and sq != sk:
        pytest.skip("causal tiles are equal-length")
    q = _rand(b, sq, n, d, dtype, 21)
    k = _rand(b, sk, n, d, dtype, 22)
    v = _rand(b, sk, n, d, dtype, 23)
    do = _rand(b, sq, n, d, dtype, 24)
    scale = 1.0 / math.sqrt(d)
    ext = _ext()
    o, lse = ext.attn_fwd(q, k, v, scale, causal)
    delta = ext.attn_bwd_preprocess(o.to(dtype), do)
    dq, dk, dv = ext.attn_bwd(do, q, k, v, delta, lse, scale, causal, False)
    # oracle with its own fp32 forward
    o_ref, lse_ref = oracle.tile_fwd(q.cpu(), k.cpu(), v.cpu(), scale, causal)
    dq_r, dk_r, dv_r = oracle.tile_bwd(
        do.cpu(), q.cpu(), k.cpu(), v.cpu(), lse_ref, scale, causal, o=o_ref
    )
    torch.testing.assert_close(dv.cpu(), dv_r, **BWD_TOL[dtype])
    torch.testing.assert_close(dk.cpu(), dk_r, **BWD_TOL[dtype])
    torch.testing.assert_close(dq.cpu(), dq_r, **BWD_TOL[dtype])


@pytest.mark.parametrize("dtype", [torch.float16])
def test_merge_two_rounds_equals_full(dtype):
    """Two half-kv tiles merged on GPU (the per-round LSE merge the ring
    does) must equal one full tile — the invariant of
    burst_attn_interface.py:214-242."""
    from burst_attn_amd.tile import HipTileProvider

    P = HipTileProvider()
    b, s, n, d = 1, 256, 2, 128
    q = _rand(b, s, n, d, dtype, 31)
    k = _rand(b, 2 * s, n, d, dtype, 32)
    v = _rand(b, 2 * s, n, d, dtype, 33)
    scale = 1.0 / math.sqrt(d)
    o1, lse1 = P.fwd(q, k[:, :s], v[:, :s], scale, False)
    o2, lse2 = P.fwd(q, k[:, s:], v[:, s:], scale, False)
    o = o1.to(torch.float32)
    lse = lse1.transpose(-2, -1).unsqueeze(-1).contiguous()
    o, lse = P.merge(o, lse, o2, lse2)
    o_full, _ = P.fwd(q, k, v, scale, False)
    torch.testing.assert_close(o, o_full, rtol=2e-3, atol=1e-2)


@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("striped", [False, True])
@pytest.mark.parametrize("causal", [False, True])
def test_interface_end_to_end_single_rank(causal, striped, d):
    """Full burst_attn_func autograd cycle on one GPU (W=1 ring) vs the
    eager full-attention oracle."""
    import torch.distributed as dist

    if not dist.is_initialized():
        import os

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29712")
        dist.init_process_group("nccl", rank=0, world_size=1)
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    b, s, n = 2, 512, 2
    dtype = torch.float16
    q = _rand(b, s, n, d, dtype, 41).requires_grad_()
    k = _rand(b, s, n, d, dtype, 42).requires_grad_()
    v = _rand(b, s, n, d, dtype, 43).requires_grad_()
    do = _rand(b, s, n, d, dtype, 44)
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(q, k, v, None, "cuda", causal)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
    o_ref, dq_r, dk_r, dv_r = oracle.ring_forward_backward_reference(
        q.detach().cpu(), k.detach().cpu(), v.detach().cpu(), do.cpu(), None, causal
    )
    tol = dict(rtol=2e-3, atol=1e-2)
    btol = dict(rtol=5e-3, atol=2e-2)
    torch.testing.assert_close(o.float().cpu(), o_ref, **tol)
    torch.testing.assert_close(dv.float().cpu(), dv_r, **btol)
    torch.testing.assert_close(dk.float().cpu(), dk_r, **btol)
    torch.testing.assert_close(dq.float().cpu(), dq_r, **btol)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_fwd_defer_max_rescale_forced(dtype):
    """The defer-max rescale branch (T13) is rare on random data — force it
    (cdna guide §5.4 rule 26): spike K rows mid-sequence so the running max
    jumps far past the defer threshold at chosen tiles, and check against
    the fp32 oracle.  A kernel that mis-scales pending state when the
    branch fires fails loudly here."""
    b, s, n, d = 1, 1024, 2, 128
    g = torch.Generator().manual_seed(77)
    q = torch.randn(b, s, n, d, generator=g)
    k = torch.randn(b, s, n, d, generator=g)
    v = torch.randn(b, s, n, d, generator=g)
    # spikes at several kv positions (different tiles), aligned with q so
    # raw q.k is huge: scores jump by ~ d * 40 / sqrt(d) >> THR
    for pos in (150, 400, 700, 1001):
        k[:, pos] = q[:, pos % 64 + 256] * 6.0
    scale = 1.0 / math.sqrt(d)
    qg, kg, vg = (t.to(dtype).cuda() for t in (q, k, v))
    o, lse = _ext().attn_fwd(qg, kg, vg, scale, False)
    o_ref, lse_ref = oracle.tile_fwd(qg.cpu(), kg.cpu(), vg.cpu(), scale, False)
    torch.testing.assert_close(o.cpu(), o_ref, **TOL[dtype])
    torch.testing.assert_close(lse.cpu(), lse_ref, **LSE_TOL)
    # causal flavour too (different masking interaction)
    o2, _ = _ext().attn_fwd(qg, kg, vg, scale, True)
    o2_ref, _ = oracle.tile_fwd(qg.cpu(), kg.cpu(), vg.cpu(), scale, True)
    torch.testing.assert_close(o2.cpu(), o2_ref, **TOL[dtype])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_accum_carry_in_matches_stateless(dtype):
    """The in-kernel carry-in merge (fwd_accum rounds + finalize) must equal
    one stateless full tile, including the row-offset window used by the
    zigzag q1 rounds."""
    from burst_attn_amd.tile import HipTileProvider

    P = HipTileProvider()
    b, s, n, d = 1, 512, 2, 128
    q = _rand(b, s, n, d, dtype, 61)
    k = _rand(b, 2 * s, n, d, dtype, 62)
    v = _rand(b, 2 * s, n, d, dtype, 63)
    scale = 1.0 / math.sqrt(d)
    st = P.fwd_accum(None, q, k[:, :s], v[:, :s], scale, False)
    st = P.fwd_accum(st, q, k[:, s:], v[:, s:], scale, False)
    o, lse = P.fwd_finalize(st, dtype)
    o_full, lse_full = _ext().attn_fwd(q, k, v, scale, False)
    torch.testing.assert_close(o.float(), o_full, **TOL[dtype])
    torch.testing.assert_close(lse, lse_full, **LSE_TOL)
    # row-offset window: extra kv merged only into rows [half:]
    half = s // 2
    st2 = P.fwd_accum(None, q, k[:, :s], v[:, :s], scale, False)
    st2 = P.fwd_accum(st2, q[:, half:], k[:, s:], v[:, s:], scale, False,
                      row_offset=half)
    o2, _ = P.fwd_finalize(st2, dtype)
    o_top, _ = _ext().attn_fwd(q[:, :half], k[:, :s], v[:, :s], scale, False)
    o_bot, _ = _ext().attn_fwd(q[:, half:], k, v, scale, False)
    torch.testing.assert_close(o2[:, :half].float(), o_top, **TOL[dtype])
    torch.testing.assert_close(o2[:, half:].float(), o_bot, **TOL[dtype])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("opt_bwd,det", [(True, False), (False, True),
                                         (True, True)])
def test_interface_flags_single_rank(opt_bwd, det, dtype):
    """optimize_bwd_comm / deterministic flag combinations end to end on
    one GPU (the W>1 flavours are covered by the gloo ring tests)."""
    import torch.distributed as dist

    if not dist.is_initialized():
        import os

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29713")
        dist.init_process_group("nccl", rank=0, world_size=1)
    from burst_attn_amd import burst_attn_func

    b, s, n, d = 1, 512, 2, 128
    q = _rand(b, s, n, d, dtype, 81).requires_grad_()
    k = _rand(b, s, n, d, dtype, 82).requires_grad_()
    v = _rand(b, s, n, d, dtype, 83).requires_grad_()
    do = _rand(b, s, n, d, dtype, 84)
    o = burst_attn_func(q, k, v, None, "cuda", True, opt_bwd, det)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
    o_ref, dq_r, dk_r, dv_r = oracle.ring_forward_backward_reference(
        q.detach().cpu(), k.detach().cpu(), v.detach().cpu(), do.cpu(), None, True
    )
    otol = TOL[dtype]
    btol = BWD_TOL[dtype]
    torch.testing.assert_close(o.float().cpu(), o_ref, **otol)
    torch.testing.assert_close(dq.float().cpu(), dq_r, **btol)
    torch.testing.assert_close(dk.float().cpu(), dk_r, **btol)
    torch.testing.assert_close(dv.float().cpu(), dv_r, **btol)


def test_backward_bitwise_deterministic():
    """deterministic=True selects the atomic-free two-pass plan: repeated
    runs must be BITWISE identical."""
    b, s, n, d = 1, 1024, 4, 128
    dtype = torch.float16
    q = _rand(b, s, n, d, dtype, 91)
    k = _rand(b, s, n, d, dtype, 92)
    v = _rand(b, s, n, d, dtype, 93)
    do = _rand(b, s, n, d, dtype, 94)
    ext = _ext()
    scale = 1.0 / math.sqrt(d)
    o, lse = ext.attn_fwd(q, k, v, scale, True)
    delta = ext.attn_bwd_preprocess(o.to(dtype), do)
    outs = [
        ext.attn_bwd(do, q, k, v, delta, lse, scale, True, True)
        for _ in range(3)
    ]
    for i in (1, 2):
        for a, b_ in zip(outs[0], outs[i]):
            assert torch.equal(a, b_), "backward is not bitwise deterministic"


@pytest.mark.parametrize("s", [768, 744])  # 744: ragged (not /32)
@pytest.mark.parametrize("plan", ["1", "2"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_bwd_alt_plans_vs_split(s, plan, causal, dtype, monkeypatch):
    """The experimental kernel plans (BA_BWD_FUSED=1 fused dK+dV, =2
    flash-attn's atomic dq plan) must agree with the default split plan —
    all accumulate fp32; the gaps are summation order, the P/dS scratch
    round trips, and the split plan's augmentation-fold constants
    (lse/delta folded as two-element T pairs — T-squared error), so the
    bf16 bound is wider than the fp16 one."""
    b, n, d = 1, 3, 128
    q = _rand(b, s, n, d, dtype, 101)
    k = _rand(b, s, n, d, dtype, 102)
    v = _rand(b, s, n, d, dtype, 103)
    do = _rand(b, s, n, d, dtype, 104)
    ext = _ext()
    scale = 1.0 / math.sqrt(d)
    o, lse = ext.attn_fwd(q, k, v, scale, causal)
    delta = ext.attn_bwd_preprocess(o.to(dtype), do)
    monkeypatch.setenv("BA_BWD_FUSED", plan)
    alt = ext.attn_bwd(do, q, k, v, delta, lse, scale, causal, False)
    monkeypatch.setenv("BA_BWD_FUSED", "0")
    split = ext.attn_bwd(do, q, k, v, delta, lse, scale, causal, True)
    tol = (dict(rtol=2e-3, atol=1e-3) if dtype == torch.float16
           else dict(rtol=1e-2, atol=8e-3))
    for f, s_, name in zip(alt, split, ("dq", "dk", "dv")):
        torch.testing.assert_close(f, s_, msg=name, **tol)


def _knob_vs_default(knob, n, nk, causal, dtype, monkeypatch):
    """(knob=1 grads, default-plan grads) on one seeded input.  S=328: two
    256-row workgroups on each axis and a ragged tail that is a multiple
    of neither 32 nor 64."""
    b, s, d = 1, 328, 128
    q = _rand(b, s, n, d, dtype, 121)
    k = _rand(b, s, nk, d, dtype, 122)
    v = _rand(b, s, nk, d, dtype, 123)
    do = _rand(b, s, n, d, dtype, 124)
    ext = _ext()
    scale = 1.0 / math.sqrt(d)
    o, lse = ext.attn_fwd(q, k, v, scale, causal)
    delta = ext.attn_bwd_preprocess(o.to(dtype), do)
    monkeypatch.setenv(knob, "1")
    alt = ext.attn_bwd(do, q, k, v, delta, lse, scale, causal, True)
    monkeypatch.delenv(knob)
    base = ext.attn_bwd(do, q, k, v, delta, lse, scale, causal, True)
    return dict(zip(("dq", "dk", "dv"), alt)), dict(zip(("dq", "dk", "dv"), base))


# test_bwd_alt_plans_vs_split's gates for the same kernel pairs
KNOB_TOL = {
    torch.float16: dict(rtol=2e-3, atol=1e-3),
    torch.bfloat16: dict(rtol=1e-2, atol=8e-3),
}


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_bwd_dk_flip_vs_default(causal, dtype, monkeypatch):
    """BA_BWD_DK_FLIP=1 swaps the split dK kernel for the flipped one and
    nothing else: dq and dv come from the same atomic-free kernels."""
    alt, base = _knob_vs_default("BA_BWD_DK_FLIP", 2, 2, causal, dtype,
                                 monkeypatch)
    assert torch.equal(alt["dq"], base["dq"]), "dq changed"
    assert torch.equal(alt["dv"], base["dv"]), "dv changed"
    torch.testing.assert_close(alt["dk"], base["dk"], **KNOB_TOL[dtype])


@pytest.mark.parametrize("n,nk", [(2, 2), (4, 2)])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_bwd_dq_pipe_vs_default(n, nk, causal, dtype, monkeypatch):
    """BA_DQ_PIPE=1 swaps the dq kernel for its DQP=1 form and nothing
    else.  N=4/Nk=2: the DQP=1 kernel indexes K/V by n / G too."""
    alt, base = _knob_vs_default("BA_DQ_PIPE", n, nk, causal, dtype,
                                 monkeypatch)
    assert torch.equal(alt["dk"], base["dk"]), "dk changed"
    assert torch.equal(alt["dv"], base["dv"]), "dv changed"
    torch.testing.assert_close(alt["dq"], base["dq"], **KNOB_TOL[dtype])


def test_bwd_rejects_unknown_plan(monkeypatch):
    """A BA_BWD_FUSED value outside {0,1,2} fails naming the knob instead
    of silently running the default plan."""
    b, s, n, d = 1, 256, 2, 128
    dtype = torch.float16
    q = _rand(b, s, n, d, dtype, 131)
    k = _rand(b, s, n, d, dtype, 132)
    v = _rand(b, s, n, d, dtype, 133)
    do = _rand(b, s, n, d, dtype, 134)
    ext = _ext()
    scale = 1.0 / math.sqrt(d)
    o, lse = ext.attn_fwd(q, k, v, scale, False)
    delta = ext.attn_bwd_preprocess(o.to(dtype), do)
    monkeypatch.setenv("BA_BWD_FUSED", "3")
    with pytest.raises(RuntimeError, match="BA_BWD_FUSED=3"):
        ext.attn_bwd(do, q, k, v, delta, lse, scale, False, True)


@pytest.mark.parametrize("det", [False, True])
def test_bwd_accum_strided_views(det):
    """bwd_accum ADDS into strided accumulator views (the zigzag
    half-slice targets): accumulating the same tile twice into a
    half-slice view must double exactly that region and leave the rest
    untouched."""
    b, s, n, d = 1, 512, 2, 128
    dtype = torch.float16
    half = s // 2
    q = _rand(b, s, n, d, dtype, 111)
    k = _rand(b, s, n, d, dtype, 112)
    v = _rand(b, s, n, d, dtype, 113)
    do = _rand(b, s, n, d, dtype, 114)
    ext = _ext()
    scale = 1.0 / math.sqrt(d)
    o, lse = ext.attn_fwd(q[:, half:], k, v, scale, False)
    delta = ext.attn_bwd_preprocess(o.to(dtype), do[:, half:])
    ref = ext.attn_bwd(do[:, half:], q[:, half:], k, v, delta, lse, scale,
                       False, det)
    dq = torch.zeros(b, s, n, d, dtype=torch.float32, device="cuda")
    dk = torch.zeros_like(dq)
    dv = torch.zeros_like(dq)
    for _ in range(2):
        ext.attn_bwd_accum(do[:, half:], q[:, half:], k, v, delta, lse,
                           scale, False, det, dq[:, half:], dk, dv)
    assert torch.all(dq[:, :half] == 0), "untouched region modified"
    torch.testing.assert_close(dq[:, half:], 2 * ref[0], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(dk, 2 * ref[1], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(dv, 2 * ref[2], rtol=1e-4, atol=1e-4)


def test_full_size_properties():
    """Size-independent invariants at the BASELINE-scale sequence length
    (s=262144; the oracle cannot run at this size in seconds, so parity at
    full size is pinned through properties — SURVEY.md §8c):
      * v = ones  => o = 1 exactly (softmax rows are normalised);
      * q = 0     => scores uniform => lse = ln(Sk) for every row.
    One head keeps the tile to ~35 TFLOP (~50 ms)."""
    b, s, n, d = 1, 262144, 1, 128
    dtype = torch.float16
    ext = _ext()
    scale = 1.0 / math.sqrt(d)
    g = torch.Generator().manual_seed(123)
    q = torch.randn(b, s, n, d, generator=g).to(dtype).cuda()
    k = torch.randn(b, s, n, d, generator=g).to(dtype).cuda()
    ones = torch.ones(b, s, n, d, dtype=dtype).cuda()
    o, lse = ext.attn_fwd(q, k, ones, scale, False)
    torch.testing.assert_close(o, torch.ones_like(o), rtol=0, atol=2e-3)
    assert torch.isfinite(lse).all()
    # q = 0 -> lse = ln(Sk) everywhere
    zq = torch.zeros(b, 4096, n, d, dtype=dtype).cuda()
    _, lse0 = ext.attn_fwd(zq, k, ones, scale, False)
    torch.testing.assert_close(
        lse0, torch.full_like(lse0, math.log(s)), rtol=1e-4, atol=1e-3
    )
    # causal flavour: row i attends i+1 keys -> lse = ln(i+1)
    _, lse_c = ext.attn_fwd(zq[:, :2048], k[:, :2048] * 0, ones[:, :2048],
                            scale, True)
    expect = torch.log(torch.arange(1, 2049, dtype=torch.float32)).cuda()
    torch.testing.assert_close(lse_c[0, 0], expect, rtol=1e-4, atol=1e-3)


def test_fwd_shape_fuzz():
    """Seeded random-shape sweep vs the oracle (alignment edges, tiny and
    tail-heavy sizes, mixed dtypes)."""
    import random

    rng = random.Random(2024)
    ext = _ext()
    for i in range(8):
        b = rng.choice([1, 2, 3])
        n = rng.choice([1, 2, 5])
        d = rng.choice([64, 128])
        sq = rng.choice([32, 96, 257, 300, 511, 640])
        sk = rng.choice([64, 96, 320, 513])
        causal = rng.random() < 0.5 and sq == sk
        dtype = rng.choice([torch.float16, torch.bfloat16])
        q = _rand(b, sq, n, d, dtype, 100 + i)
        k = _rand(b, sk, n, d, dtype, 200 + i)
        v = _rand(b, sk, n, d, dtype, 300 + i)
        scale = 1.0 / math.sqrt(d)
        o, lse = ext.attn_fwd(q, k, v, scale, causal)
        o_ref, lse_ref = oracle.tile_fwd(q.cpu(), k.cpu(), v.cpu(), scale, causal)
        case = f"case {i}: b={b} sq={sq} sk={sk} n={n} d={d} causal={causal}"
        torch.testing.assert_close(
            o.cpu(), o_ref, msg=lambda m: f"{case}\n{m}", **TOL[dtype]
        )


def test_error_paths(monkeypatch):
    """The binding layer fails loudly on contract violations."""
    q = _rand(1, 128, 2, 128, torch.float16, 1)
    ext = _ext()
    with pytest.raises(RuntimeError):  # causal needs Sq == Sk
        ext.attn_fwd(q[:, :64], q, q, 0.1, True)
    with pytest.raises(RuntimeError):  # unsupported head_dim
        bad = _rand(1, 128, 2, 96, torch.float16, 2)
        ext.attn_fwd(bad, bad, bad, 0.1, False)
    with pytest.raises(RuntimeError):  # fp32 inputs rejected
        f32 = torch.randn(1, 128, 2, 128).cuda()
        ext.attn_fwd(f32, f32, f32, 0.1, False)
    # a knob value outside its accepted set names the knob, in both forms
    acc = torch.empty(1, 128, 2, 128, dtype=torch.float32, device="cuda")
    m = torch.empty(1, 2, 128, dtype=torch.float32, device="cuda")
    l = torch.empty(1, 2, 128, dtype=torch.float32, device="cuda")
    monkeypatch.setenv("BA_FWD_SUBT", "7")
    with pytest.raises(RuntimeError, match="BA_FWD_SUBT=7"):
        ext.attn_fwd(q, q, q, 0.1, False)
    with pytest.raises(RuntimeError, match="BA_FWD_SUBT=7"):
        ext.attn_fwd_accum(q, q, q, 0.1, False, acc, m, l, False)
    monkeypatch.delenv("BA_FWD_SUBT")
    # the previous failure left a causal-shape / bad-knob message behind:
    # the accum form's unsupported-head-dim error must carry its own
    with pytest.raises(RuntimeError, match="unsupported head_dim 96"):
        acc96 = torch.empty(1, 128, 2, 96, dtype=torch.float32, device="cuda")
        ext.attn_fwd_accum(bad, bad, bad, 0.1, False, acc96, m, l, False)
    ext.attn_fwd(q, q, q, 0.1, False)  # and the knob is read per call
    # flash="math" layout is not supported at the API layer
    import torch.distributed as dist

    if not dist.is_initialized():
        import os

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29714")
        dist.init_process_group("nccl", rank=0, world_size=1)
    from burst_attn_amd import burst_attn_func

    with pytest.raises(ValueError):
        burst_attn_func(q, q, q, None, "math")


@pytest.mark.timeout(600)
def test_large_size_direct_parity():
    """Direct (non-property) parity at s=8192 — two orders of magnitude
    above the per-case tile tests; the oracle runs blockwise on CPU in
    ~tens of seconds."""
    b, s, n, d = 1, 8192, 2, 128
    dtype = torch.float16
    q = _rand(b, s, n, d, dtype, 71)
    k = _rand(b, s, n, d, dtype, 72)
    v = _rand(b, s, n, d, dtype, 73)
    do = _rand(b, s, n, d, dtype, 74)
    scale = 1.0 / math.sqrt(d)
    ext = _ext()
    o, lse = ext.attn_fwd(q, k, v, scale, True)
    delta = ext.attn_bwd_preprocess(o.to(dtype), do)
    dq, dk, dv = ext.attn_bwd(do, q, k, v, delta, lse, scale, True, False)
    o_ref, lse_ref = oracle.tile_fwd(q.cpu(), k.cpu(), v.cpu(), scale, True,
                                     q_block=1024, k_block=1024)
    torch.testing.assert_close(o.cpu(), o_ref, **TOL[dtype])
    torch.testing.assert_close(lse.cpu(), lse_ref, **LSE_TOL)
    dq_r, dk_r, dv_r = oracle.tile_bwd(do.cpu(), q.cpu(), k.cpu(), v.cpu(),
                                       lse_ref, scale, True, o=o_ref,
                                       q_block=1024, k_block=1024)
    torch.testing.assert_close(dv.cpu(), dv_r, **BWD_TOL[dtype])
    torch.testing.assert_close(dk.cpu(), dk_r, **BWD_TOL[dtype])
    torch.testing.assert_close(dq.cpu(), dq_r, **BWD_TOL[dtype])


@pytest.mark.parametrize("asm", ["1", "2"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_asm_module_fwd_parity(asm, dtype, monkeypatch):
    """The .s-assembled hipModule forward (BA_FWD_ASM) vs the in-binary
    kernel.  asm=1 is the unmodified re-assembly and must be BITWISE
    identical (same instructions, same launch); asm=2 is the
    tools/s_patch.py qk_split variant, which reorders the in-D summation
    (two partial accumulators) and gates at the tile tolerance."""
    from burst_attn_amd.tile import HipTileProvider

    base = HipTileProvider()          # plain extension dispatch
    monkeypatch.setenv("BA_FWD_ASM", asm)
    pa = HipTileProvider()            # module dispatch
    assert pa._asm_fwd
    scale = 1.0 / math.sqrt(128)
    for b, s, n, causal, seed in [(1, 1024, 4, False, 70), (1, 744, 2, True, 71),
                                  (2, 512, 3, False, 72)]:
        q = _rand(b, s, n, 128, dtype, seed)
        k = _rand(b, s, n, 128, dtype, seed + 100)
        v = _rand(b, s, n, 128, dtype, seed + 200)
        st_a = pa.fwd_accum(None, q, k, v, scale, causal)
        st_b = base.fwd_accum(None, q, k, v, scale, causal)
        if asm == "1":
            for ta, tb in zip(st_a, st_b):
                assert torch.equal(ta, tb), "re-assembly must be bitwise equal"
        else:
            o_a, lse_a = pa.fwd_finalize(st_a, dtype)
            o_b, lse_b = base.fwd_finalize(st_b, dtype)
            torch.testing.assert_close(o_a.float(), o_b.float(), **TOL[dtype])
            torch.testing.assert_close(lse_a, lse_b, **LSE_TOL)
    # D=64 falls back to the in-binary kernel rather than failing
    q = _rand(1, 256, 2, 64, dtype, 80)
    k = _rand(1, 256, 2, 64, dtype, 81)
    v = _rand(1, 256, 2, 64, dtype, 82)
    st = pa.fwd_accum(None, q, k, v, 0.125, False)
    st_ref = base.fwd_accum(None, q, k, v, 0.125, False)
    for ta, tb in zip(st, st_ref):
        assert torch.equal(ta, tb)


FWD_ALT_KNOBS = pytest.mark.parametrize("knobs", [
    {"BA_FWD_SUBT": "2", "BA_FWD_NBUF": "4"},   # T15 double-pipeline
    {"BA_FWD_SUBT": "3", "BA_FWD_NBUF": "4"},   # 3-stage 1-wave scaffold
    {"BA_FWD_NBUF": "4"},                        # 4-buffer staging
    {"BA_FWD_VPATH": "1"},                       # tr16 V path
    {"BA_FWD_SUBT": "0"},                        # joint softmax
    {"BA_FWD_KREG": "1"},                        # K straight to registers
    {"BA_FWD_KREG": "2"},                        # K-fragment prefetch
    {"BA_FWD_NT": "256"},                        # 4-wave workgroups
], ids=["subt2", "subt3", "nbuf4", "vpath1", "subt0", "kreg1", "kreg2",
        "nt256"])


@FWD_ALT_KNOBS
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_fwd_alt_paths_vs_default(knobs, causal, dtype, monkeypatch):
    """Every env-selectable forward variant must agree with the default
    path (the launcher reads the knobs per call, so this runs in-process
    like the backward-plan test).  Ragged sizes included: the variants
    share masking/boundary code but differ in staging and softmax
    structure, where boundary bugs would hide."""
    ext = _ext()
    scale = 1.0 / math.sqrt(128)
    for s, seed in ((768, 130), (744, 131)):
        q = _rand(1, s, 2, 128, dtype, seed)
        k = _rand(1, s, 2, 128, dtype, seed + 10)
        v = _rand(1, s, 2, 128, dtype, seed + 20)
        o_ref, lse_ref = ext.attn_fwd(q, k, v, scale, causal)
        for key, val in knobs.items():
            monkeypatch.setenv(key, val)
        o_alt, lse_alt = ext.attn_fwd(q, k, v, scale, causal)
        for key in knobs:
            monkeypatch.delenv(key)
        torch.testing.assert_close(o_alt, o_ref, **TOL[dtype])
        torch.testing.assert_close(lse_alt, lse_ref, **LSE_TOL)


def _carry_in_two_halves(q, k, v, scale, dtype):
    """fresh accum on the first kv half, carry-in on the second, finalize."""
    ext = _ext()
    b, sq, n, d = q.shape
    half = k.shape[1] // 2
    acc = torch.empty(b, sq, n, d, dtype=torch.float32, device=q.device)
    m = torch.empty(b, n, sq, dtype=torch.float32, device=q.device)
    l = torch.empty(b, n, sq, dtype=torch.float32, device=q.device)
    ext.attn_fwd_accum(q, k[:, :half], v[:, :half], scale, False, acc, m, l,
                       False)
    ext.attn_fwd_accum(q, k[:, half:], v[:, half:], scale, False, acc, m, l,
                       True)
    return ext.attn_fwd_finalize(acc, m, l, dtype)


_CARRY_IN_DEFAULT = {}


@FWD_ALT_KNOBS
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_fwd_alt_paths_carry_in_vs_default(knobs, dtype, monkeypatch):
    """The same knob sets through the carry-in kernel (OUT_STATE=1), the
    form the ring runs: ragged s_q=744 against two 384-row kv halves, so
    the second call merges into carried state across a ragged q tail."""
    scale = 1.0 / math.sqrt(128)
    if dtype not in _CARRY_IN_DEFAULT:
        q = _rand(1, 744, 2, 128, dtype, 140)
        k = _rand(1, 768, 2, 128, dtype, 141)
        v = _rand(1, 768, 2, 128, dtype, 142)
        _CARRY_IN_DEFAULT[dtype] = (
            q, k, v, _carry_in_two_halves(q, k, v, scale, dtype))
    q, k, v, (o_ref, lse_ref) = _CARRY_IN_DEFAULT[dtype]
    for key, val in knobs.items():
        monkeypatch.setenv(key, val)
    o_alt, lse_alt = _carry_in_two_halves(q, k, v, scale, dtype)
    torch.testing.assert_close(o_alt.float(), o_ref.float(), **TOL[dtype])
    torch.testing.assert_close(lse_alt, lse_ref, **LSE_TOL)


def _d64_both_forms(q, ka, va, kb, vb, scale, causal, dtype):
    """The stateless tile on (ka, va), and the two-call carry-in form: a
    fresh accumulator on (ka, va) under the mask, then (kb, vb) unmasked
    merged in-kernel and finalized, the way a ring's diagonal round is
    followed by a full one."""
    ext = _ext()
    o, lse = ext.attn_fwd(q, ka, va, scale, causal)
    b, sq, n, d = q.shape
    acc = torch.empty(b, sq, n, d, dtype=torch.float32, device=q.device)
    m = torch.empty(b, n, sq, dtype=torch.float32, device=q.device)
    l = torch.empty(b, n, sq, dtype=torch.float32, device=q.device)
    ext.attn_fwd_accum(q, ka, va, scale, causal, acc, m, l, False)
    ext.attn_fwd_accum(q, kb, vb, scale, False, acc, m, l, True)
    o_c, lse_c = ext.attn_fwd_finalize(acc, m, l, dtype)
    return o, lse, o_c, lse_c


_D64_DEFAULT = {}


@FWD_ALT_KNOBS
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_fwd_alt_paths_d64_vs_default(knobs, causal, dtype, monkeypatch):
    """The knob sets at head_dim 64 (the tests above run them at 128 only),
    stateless and carry-in, against the default variant.  Sq = Sk = 296:
    five kv tiles, so NBUF=4 wraps; the last one a ragged 40 rows; a ragged
    q tail for both NT=512 and NT=256; N=4 over Nk=2 keeps the grouped-query
    head mapping live."""
    scale = 1.0 / math.sqrt(64)
    if (dtype, causal) not in _D64_DEFAULT:
        q = _rand(1, 296, 4, 64, dtype, 150)
        kv = [_rand(1, 296, 2, 64, dtype, 151 + i) for i in range(4)]
        _D64_DEFAULT[dtype, causal] = (
            q, kv, _d64_both_forms(q, *kv, scale, causal, dtype))
    q, kv, ref = _D64_DEFAULT[dtype, causal]
    for key, val in knobs.items():
        monkeypatch.setenv(key, val)
    alt = _d64_both_forms(q, *kv, scale, causal, dtype)
    for (o_alt, lse_alt), (o_ref, lse_ref) in ((alt[:2], ref[:2]),
                                               (alt[2:], ref[2:])):
        torch.testing.assert_close(o_alt.float(), o_ref.float(), **TOL[dtype])
        torch.testing.assert_close(lse_alt, lse_ref, **LSE_TOL)
