"""The head_dim 256, 192 / 128 and fp8 kernel sets in the forms the ring's
rounds give them, on ONE GPU.

tests/test_gpu_ring_rounds.py replays whole W = 3 / 4 rings through the
64- and 128-wide kernels.  The three later sets are separate code with
128-row workgroups, launchers and epilogues of their own, and all ship in
``burst_attn_func`` at W > 1; here ``ring_rounds.replay_ring`` (16-bit) and
``ring_rounds.replay_ring_fp8`` (forward only) drive ``HipTileProvider``
through the same calls on ``ring_rounds.SET_CASES``: causal carry-in rounds,
the zigzag ``row_offset = half`` windows (half = 165, odd), the striped
one-token shift, and ``bwd_accum`` under the whole-sequence lse and delta
into accumulators shared by W rounds (dv in v's shape, 128 wide under a
192-wide dk).

d256 and hd192: reference and gates are those of test_gpu_ring_rounds.py,
the fp32 full-sequence oracle (``gqa_full_reference``, which takes o's
width from v; ``mutant_oracle.forward`` for lse) and
``boundary_refs.gates``; causal cases run the stateless form first.

fp8, per-tensor: the exact-P needle (``ring_rounds.fp8_needle``) is the
sharp gate, every P a power of two, held to TOL[fp16] and LSE_TOL against
fp64 attention on the dequantised inputs; the quantised ``diag_needle`` is
held to the bound of tests/test_gpu_fp8.py::test_quantised_realistic on
the full sequence.  fp8, block-scaled: power-of-two scales per rank, row,
tile, channel, head and batch, held to the bound of
tests/test_gpu_fp8_scaled.py; the calls carry ``dq[:, :, qw]`` (strided for
the zigzag later half and the striped shift) and the source rank's dk
tiles, which start at tile 3 for a zigzag later half at s_local = 384.

tests/test_ring_sets_cpu.py proves on the CPU that on these cases the
gates reject a one-pair or one-row error in any of those forms.

Every check prints ``GATE ring-sets[-stateless] <case> <dtype> <output>
<ratio>`` (shown under ``-s``); profiles/gate_sensitivity/README.md records
them.
"""

import functools
import math

import pytest
import torch

from . import mutant_oracle as mo
from . import ring_rounds as rr
from .boundary_inputs import dtype_name as _dt
from .boundary_refs import gates
from .gqa_cpu_provider import gqa_full_reference
from .ring_sim import simulate_ring
from .test_gpu_parity import LSE_TOL, TOL

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
F16 = TOL[torch.float16]
CASES_16 = [c for c in rr.SET_CASES if c.kset in ("d256", "hd192")]
# both values of `deterministic` at W = 4, lag 0; (case, dtype) varies
# slowest, so the shared reference is computed once and then dropped
PARAMS = [(c, t, det) for c in CASES_16 for t in DTYPES
          for det in ((False, True) if (c.W, c.lag, c.causal) == (4, 0, True)
                      else (False,))]
RING = pytest.mark.parametrize(
    "case,dtype,det", PARAMS,
    ids=[f"{rr.case_id(c)}-{_dt(t)}-{'det' if det else 'atomic-ok'}"
         for c, t, det in PARAMS])


def _provider():
    from burst_attn_amd.tile import HipTileProvider

    return HipTileProvider()


@functools.lru_cache(maxsize=2)
def _reference(case, dtype):
    """fp32 full-sequence (o, lse, dq, dk, dv) on the CPU; never modified."""
    q, k, v, do = rr.make_inputs(case, dtype)
    scale = rr.scale_of(case)
    o, dq, dk, dv = gqa_full_reference(q, k, v, do, scale, case.causal)
    S = q.shape[1]
    lse = mo.forward(q, k, v, scale, mo.base_spec(
        mo.Ctx(case.b, S, S, case.n, case.nk, case.causal)))[1]
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def _check(case, dtype, forms):
    gt = gates(dtype, case.n // case.nk)
    refs = _reference(case, dtype)
    triples = [(test, name, out.float().cpu())
               for test, outs in forms for name, out in outs.items()]
    for test, name, out in triples:
        print(f"GATE {test} {rr.case_id(case)} {_dt(dtype)} {name} "
              f"{mo.gate_ratio(out, refs[name], **gt[name]):.3f}")
    for test, name, out in triples:
        assert out.shape == refs[name].shape, (test, name, out.shape)
        torch.testing.assert_close(
            out, refs[name], msg=lambda m: f"{test} {name}: {m}", **gt[name])


@RING
def test_ring_rounds_16bit(case, dtype, det):
    P = _provider()
    q, k, v, do = (t.cuda() for t in rr.make_inputs(case, dtype))
    scale = rr.scale_of(case)
    got = rr.replay_ring(P, q, k, v, do, case.W, scale, case.causal,
                         case.layout, deterministic=det)
    accum = dict(zip(("o", "lse", "dq", "dk", "dv"), got))
    assert accum["dk"].shape == k.shape and accum["dv"].shape == v.shape
    forms = []
    if case.causal and not det:  # simulate_ring's backward has no det flag
        o, dq, dk, dv, lse = simulate_ring(
            P, q, k, v, do, case.W, scale, True,
            striped=case.layout == "striped", return_lse=True)
        # asserted first: if it fails too, the tile itself is wrong
        forms.append(("ring-sets-stateless",
                      {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}))
    _check(case, dtype, forms + [("ring-sets", accum)])


# ---- fp8: forward only

def _attn64(qd, kd, vd, scale, causal):
    """fp64 (o, lse [B,N,S], P @ |V|, sum_j |v_jd|) of double q, k, v."""
    g = qd.shape[2] // kd.shape[2]
    ke, ve = (t.repeat_interleave(g, dim=2) for t in (kd, vd))
    s = torch.einsum("bqnd,bknd->bnqk", qd, ke) * scale
    if causal:
        s = s.masked_fill(~torch.ones(s.shape[-2:], dtype=torch.bool).tril(),
                          -math.inf)
    p = torch.softmax(s, -1)
    return (torch.einsum("bnqk,bknd->bqnd", p, ve), torch.logsumexp(s, -1),
            torch.einsum("bnqk,bknd->bqnd", p, ve.abs()),
            ve.abs().sum(1, keepdim=True))


@functools.lru_cache(maxsize=1)
def _fp8_reference(case):
    *_, scale, deq = rr.make_fp8_inputs(case)
    return _attn64(*deq, scale, case.causal)


def _fp8_replay(case, out_dtype=torch.float16):
    q8, k8, v8, ds, scale, _ = rr.make_fp8_inputs(case)
    if not isinstance(ds, tuple):
        ds = [tuple(t.cuda() for t in rank) for rank in ds]
    return rr.replay_ring_fp8(_provider(), q8.cuda(), k8.cuda(), v8.cuda(),
                              case.W, scale, case.causal, case.layout, ds,
                              out_dtype)


def _cases_of(kset, family):
    return pytest.mark.parametrize(
        "case", [c for c in rr.SET_CASES
                 if (c.kset, c.family) == (kset, family)], ids=rr.case_id)


@_cases_of("fp8", "fp8_needle")
def test_ring_rounds_fp8_exact_p(case):
    """Every P is a power of two: the 16-bit gates apply unchanged."""
    o, lse = _fp8_replay(case)
    ref = _fp8_reference(case)
    outs = {"o": (o, ref[0].float(), F16), "lse": (lse, ref[1].float(),
                                                   LSE_TOL)}
    for name, (out, r, gate) in outs.items():
        print(f"GATE ring-sets {rr.case_id(case)} fp8 {name} "
              f"{mo.gate_ratio(out.float().cpu(), r, **gate):.3f}")
    for name, (out, r, gate) in outs.items():
        torch.testing.assert_close(out.float().cpu(), r,
                                   msg=lambda m: f"{name}: {m}", **gate)


@_cases_of("fp8", "fp8_realistic")
def test_ring_rounds_fp8_realistic(case):
    """lse at LSE_TOL; o within TOL[fp16] plus the worst case of rounding P
    to e4m3, the bound of test_gpu_fp8.py::test_quantised_realistic, here
    over the full sequence."""
    p = _provider()
    o, lse = _fp8_replay(case)
    o64, lse64, pv, vsum = (t.float() for t in _fp8_reference(case))
    print(f"GATE ring-sets {rr.case_id(case)} fp8 lse "
          f"{mo.gate_ratio(lse.cpu(), lse64, **LSE_TOL):.3f}")
    c = p._ext.attn_fp8_p_scale()
    bound = (F16["atol"] + F16["rtol"] * o64.abs() + 2.0 ** -4 * pv
             + (2.0 ** -10 / c) * vsum)
    err = (o.float().cpu() - o64).abs()
    print(f"GATE ring-sets {rr.case_id(case)} fp8 o(max |err| / bound) "
          f"{float((err / bound).max()):.3f}")
    torch.testing.assert_close(lse.cpu(), lse64, **LSE_TOL)
    assert bool((err <= bound).all())


@_cases_of("fp8_scaled", "fp8_pow2")
def test_ring_rounds_fp8_scaled(case):
    """The _within bound of tests/test_gpu_fp8_scaled.py on the full
    sequence (c = 16 is the kernel's P scale)."""
    o, _ = _fp8_replay(case)
    o64, _, pv, vsum = _fp8_reference(case)
    bound = 1e-2 + 2e-3 * o64.abs() + 2.0 ** -4 * pv + 2.0 ** -10 / 16 * vsum
    err = (o.double().cpu() - o64).abs()
    print(f"GATE ring-sets {rr.case_id(case)} fp8 o(max |err| / bound) "
          f"{float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
