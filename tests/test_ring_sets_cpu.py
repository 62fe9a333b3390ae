"""CPU proof for tests/test_gpu_ring_sets.py: the fp8 replay is right, and
on ``ring_rounds.SET_CASES`` the gates see an error confined to one ring
seam.  Mutants, scoring, CAUGHT / CLEAN and the (empty) NOT_SEPARABLE list
are those of tests/test_ring_rounds_cpu.py.

(a) ``ring_rounds.replay_ring_fp8`` with an oracle provider that
    dequantises by the descales it is handed equals fp64 attention on the
    dequantised full sequence, per-tensor and block-scaled (each rank's
    chunk by its own dq, dk tiles and dv), both layouts.

(b) head_dim 256 and 192 / 128: on every 16-bit case the rounding emulation
    of the unmutated math scores <= CLEAN on every output, and every window
    and replay mutant scores >= CAUGHT on at least one output in at least
    one case of its kernel set and layout.

(c) fp8 exact-P needle, in fp32 on the dequantised inputs, against
    TOL[fp16] / LSE_TOL: every window mutant and every replay mutant of the
    forward (row_offset+-1, carry_ignored; the fp8 kernels have no
    backward) moves o or lse by >= CAUGHT in at least one case of its
    layout; the unmutated math with P rounded to e4m3 at the kernel's P
    scale of 16 and o to fp16 scores <= CLEAN on every case.
"""

import dataclasses
import functools
import math

import pytest
import torch

from . import mutant_oracle as mo
from . import ring_rounds as rr
from .boundary_inputs import dtype_name as _dt
from .gqa_cpu_provider import GqaOracleTileProvider
from .test_gate_sensitivity_cpu import CAUGHT, CLEAN
from .test_gpu_parity import LSE_TOL, TOL
from .test_ring_rounds_cpu import (NOT_SEPARABLE, REPLAY_MUTANTS,
                                   WINDOW_MUTANTS, FaultyProvider, _allow,
                                   evaluate, mutants_of)

DTYPES = [torch.float16, torch.bfloat16]
CASES_16 = [c for c in rr.SET_CASES if c.kset in ("d256", "hd192")]
NEEDLE = [c for c in rr.SET_CASES if c.family == "fp8_needle"]
FWD_REPLAY_MUTANTS = ("row_offset+1", "row_offset-1", "carry_ignored")


def _dequantising(base):
    """`base` with fwd_accum taking fp8 inputs and descale= floats or
    tensors (dq [B,N,Sq], dk [B,Nk,tiles], dv [B,Nk,D])."""

    class Provider(base):
        def fwd_accum(self, state, q, k, v, scale, causal, row_offset=0,
                      descale=None):
            dq, dk, dv = descale
            if isinstance(dq, torch.Tensor):
                dq = dq.transpose(1, 2)[..., None]
                dk = dk.repeat_interleave(64, 2)[:, :, :k.shape[1]].transpose(
                    1, 2)[..., None]
                dv = dv[:, None]
            return super().fwd_accum(state, q.float() * dq, k.float() * dk,
                                     v.float() * dv, scale, causal,
                                     row_offset)

    return Provider


def _attn(qd, kd, vd, scale, allow):
    spec = mo.base_spec(mo.Ctx(qd.shape[0], qd.shape[1], kd.shape[1],
                               qd.shape[2], kd.shape[2], False))
    return mo.forward(qd.float(), kd.float(), vd.float(), scale,
                      dataclasses.replace(spec, allow=allow))


# ---- (a)

@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("kset,family,layout,s_local", [
    ("fp8", "fp8_needle", "zigzag", 70), ("fp8", "fp8_needle", "striped", 70),
    ("fp8_scaled", "fp8_pow2", "zigzag", 256),
    ("fp8_scaled", "fp8_pow2", "striped", 70)])
def test_fp8_replay_equals_full_sequence(kset, family, layout, s_local, W,
                                         causal):
    case = rr.SetCase(kset, family, layout, W, 2, s_local, 4, 2, 128, 128, 1,
                      causal)
    q8, k8, v8, ds, scale, deq = rr.make_fp8_inputs(case)
    P = _dequantising(GqaOracleTileProvider)()
    o, lse = rr.replay_ring_fp8(P, q8, k8, v8, W, scale, causal, layout, ds,
                                torch.float32)
    S = W * s_local
    allow = torch.ones(S, S, dtype=torch.bool)
    o_r, lse_r = _attn(*deq, scale, allow.tril() if causal else allow)
    torch.testing.assert_close(o, o_r, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(lse, lse_r, rtol=1e-4, atol=1e-4)
    if kset == "fp8_scaled":  # the scales differ by rank, tile and row
        assert len({tuple(t.flatten().tolist()) for t in
                    (r[1] for r in ds)}) == W


# ---- (b)

@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("case", CASES_16, ids=rr.case_id)
def test_rounding_emulation_passes(case, dtype):
    over = {k: r for k, r in evaluate(case, dtype)["emu"].items()
            if r > CLEAN}
    assert not over, over


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("layout", ["zigzag", "striped"])
@pytest.mark.parametrize("kset", ["d256", "hd192"])
def test_mutants_rejected(kset, layout, dtype):
    assert not NOT_SEPARABLE  # nothing is excused here either
    cases = [c for c in CASES_16 if (c.kset, c.layout) == (kset, layout)]
    missed = {}
    for mutant in tuple(WINDOW_MUTANTS[layout]) + REPLAY_MUTANTS:
        best = max(max(evaluate(c, dtype)[mutant].values()) for c in cases
                   if mutant in mutants_of(c))
        if best < CAUGHT:
            missed[mutant] = best
    assert not missed, missed


# ---- (c)

_GATES = {"o": TOL[torch.float16], "lse": LSE_TOL}


def _score(o, lse, ref):
    return {"o": mo.gate_ratio(o, ref[0], **_GATES["o"]),
            "lse": mo.gate_ratio(lse, ref[1], **_GATES["lse"])}


def _p8_forward(qd, kd, vd, scale, allow, p_scale=16.0):
    """The forward with P = exp2(s - max) rounded to e4m3 at the kernel's
    P scale and o rounded to fp16; l stays the fp32 sum."""
    g = qd.shape[2] // kd.shape[2]
    ke, ve = (t.float().repeat_interleave(g, dim=2) for t in (kd, vd))
    s = torch.einsum("bqnd,bknd->bnqk", qd.float(), ke) * scale
    s = s.masked_fill(~allow, -math.inf)
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    p8 = (p * p_scale).to(rr.FP8).float() / p_scale
    o = torch.einsum("bnqk,bknd->bqnd", p8, ve) / p.sum(-1).transpose(
        1, 2)[..., None]
    return o.half().float(), (m.squeeze(-1) + torch.log(p.sum(-1)))


@functools.lru_cache(maxsize=None)
def evaluate_needle(case):
    q8, k8, v8, ds, scale, deq = rr.make_fp8_inputs(case)
    tril = _allow(case.layout, case.W, case.s_local)
    ref = _attn(*deq, scale, tril)
    out = {"emu": _score(*_p8_forward(*deq, scale, tril), ref)}
    for name in WINDOW_MUTANTS[case.layout]:
        out[name] = _score(*_attn(*deq, scale, _allow(
            case.layout, case.W, case.s_local, name)), ref)
    for name in FWD_REPLAY_MUTANTS:
        P = _dequantising(FaultyProvider)(name)
        out[name] = _score(*rr.replay_ring_fp8(
            P, q8, k8, v8, case.W, scale, True, case.layout, ds,
            torch.float32), ref)
    return out


@pytest.mark.parametrize("case", NEEDLE, ids=rr.case_id)
def test_needle_scores_are_integers_within_span(case):
    """What makes P exact: integer exp2-domain scores whose span under the
    causal mask keeps P * 16 an e4m3 value."""
    *_, scale, (qd, kd, _) = rr.make_fp8_inputs(case)
    s = torch.einsum("bqnd,bknd->bnqk", qd[:, :, :1], kd[:, :, :1])
    assert scale == math.log(2.0) and torch.equal(s, s.round())
    assert float(s.max() - s.min()) == rr.FP8_NEEDLE_SPAN <= 12


@pytest.mark.parametrize("case", NEEDLE, ids=rr.case_id)
def test_needle_emulation_passes(case):
    over = {k: r for k, r in evaluate_needle(case)["emu"].items()
            if r > CLEAN}
    assert not over, over


@pytest.mark.parametrize("layout", ["zigzag", "striped"])
def test_needle_mutants_rejected(layout):
    cases = [c for c in NEEDLE if c.layout == layout]
    missed = {}
    for mutant in tuple(WINDOW_MUTANTS[layout]) + FWD_REPLAY_MUTANTS:
        best = max(max(evaluate_needle(c)[mutant].values()) for c in cases)
        if best < CAUGHT:
            missed[mutant] = best
    assert not missed, missed
