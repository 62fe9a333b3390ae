"""GPU parity on inputs whose softmax mass sits on the kernels' seams.

The kernels run on the families of tests/boundary_inputs.py and are held
to the CPU oracle (``oracle.tile_fwd`` / ``oracle.tile_bwd``; grouped
heads through tests/gqa_cpu_provider.py's expand / reduce, dk/dv at G x
atol) by the unchanged gates of tests/test_gpu_parity.py.  On randn inputs
those gates pass an error confined to a few (row, key) pairs; on these
they reject it.  tests/test_gate_sensitivity_cpu.py proves that on the CPU
for the cases run here (``boundary_inputs.CASES``): the stateless forward,
the two-call carry-in form with the same second-round keys
(``boundary_inputs.round2_kv``), and the backward, with the two exceptions
its docstring lists.  The poisoned-parent tests reuse the same tensors.

The ring's later rounds hand the kernels forms of their own, run here at
tile level on the same cases (tests/test_gpu_ring_rounds.py runs whole
rings of them): the causal carry-in call, the call on views shifted by
one token, the rescale of carried state by a round that dominates it or
is dominated by it, and the backward under an lse and delta that belong to
more keys than the tile's.

Every forward knob set of FWD_ALT_KNOBS (test_gpu_parity.py) and every
backward knob of BWD_KNOBS below is run against the oracle at S=328, at
head_dim 64 and 128 (separate kernel instantiations); a new knob value
belongs in one of the two lists.

Each check prints ``GATE <test> <case> <dtype> <output> <ratio>`` (shown
under ``-s``): the worst max |err| / (atol + rtol |ref|) of that output.
profiles/gate_sensitivity/README.md records them.
"""

import pytest
import torch

from . import boundary_inputs as bi
from .boundary_inputs import case_id as _id, dtype_name as _dt
from .boundary_refs import (bwd_ref as _bwd_ref, carry_ref as _carry_ref,
                            dominated_kv as _dominated_kv,
                            dominated_ref as _dominated_ref,
                            fwd_ref as _fwd_ref, gates, inputs as _inputs,
                            merged_bwd_ref as _merged_bwd_ref,
                            round2_kv as _round2_kv, scale_of as _scale,
                            shifted_ref as _shifted_ref)
from .mutant_oracle import gate_ratio
from .test_gpu_parity import FWD_ALT_KNOBS

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
CASES = pytest.mark.parametrize("case", bi.CASES, ids=_id)
KNOB_CASES = pytest.mark.parametrize("case", bi.KNOB_CASES, ids=_id)
BY_DTYPE = pytest.mark.parametrize("dtype", DTYPES, ids=_dt)


def _ext():
    from burst_attn_amd._ext import load_extension

    return load_extension()


def _gpu(*ts):
    return tuple(t.cuda() for t in ts)


def _check(test, case, dtype, outs, refs):
    """Print every output's worst gate ratio, then assert the gates (a
    second round's dk2/dv2 under the dk/dv gates)."""
    gt = gates(dtype, case.n // case.nk)
    gt.update(dk2=gt["dk"], dv2=gt["dv"])
    pairs = [(name, outs[name].float().cpu(), refs[name]) for name in outs]
    for name, out, ref in pairs:
        print(f"GATE {test} {_id(case)} {_dt(dtype)} {name} "
              f"{gate_ratio(out, ref, **gt[name]):.3f}")
    for name, out, ref in pairs:
        torch.testing.assert_close(out, ref, msg=lambda m: f"{name}: {m}",
                                   **gt[name])


# ---- forward

def _stateless(case, dtype):
    q, k, v, _ = _gpu(*_inputs(case, dtype))
    o, lse = _ext().attn_fwd(q, k, v, _scale(case), case.causal)
    return {"o": o, "lse": lse}


def _state(b, sq, n, d):
    acc = torch.empty(b, sq, n, d, dtype=torch.float32, device="cuda")
    m = torch.empty(b, n, sq, dtype=torch.float32, device="cuda")
    return acc, m, torch.empty_like(m)


def _carry_in(case, dtype):
    """A fresh accumulator on (k, v) under the case's mask, then round 2
    unmasked merged in-kernel, then finalize: a ring's diagonal round
    followed by a full one (test_gpu_parity._d64_both_forms)."""
    ext = _ext()
    q, k, v, _ = _gpu(*_inputs(case, dtype))
    k2, v2 = _gpu(*_round2_kv(case, dtype))
    acc, m, l = _state(case.b, case.sq, case.n, case.d)
    ext.attn_fwd_accum(q, k, v, _scale(case), case.causal, acc, m, l, False)
    ext.attn_fwd_accum(q, k2, v2, _scale(case), False, acc, m, l, True)
    o, lse = ext.attn_fwd_finalize(acc, m, l, dtype)
    return {"o": o, "lse": lse}


def _named(o_lse):
    return dict(zip(("o", "lse"), o_lse))


@BY_DTYPE
@CASES
def test_fwd_stateless(case, dtype):
    _check("fwd", case, dtype, _stateless(case, dtype),
           _named(_fwd_ref(case, dtype)))


@BY_DTYPE
@CASES
def test_fwd_carry_in(case, dtype):
    _check("carry", case, dtype, _carry_in(case, dtype),
           _named(_carry_ref(case, dtype)))


# ---- forward: the carry-in forms of the ring's later rounds.  The striped
# ring's rounds 2..W are CAUSAL carry-in calls, half of them on views
# shifted by one token, whose m/l rows start 4 bytes into the parent's.

CAUSAL_CASES = pytest.mark.parametrize(
    "case", [c for c in bi.CASES if c.causal], ids=_id)
SHIFT_CASES = pytest.mark.parametrize(
    "case", [c for c in bi.CASES if c.causal and c.sq >= 2], ids=_id)


@BY_DTYPE
@CAUSAL_CASES
def test_fwd_carry_in_causal(case, dtype):
    """The striped order, the reverse of _carry_in: a fresh unmasked round
    on round2_kv, then the case's keys merged in under the causal mask.
    The merge does not depend on the order, so the reference is the same."""
    ext = _ext()
    q, k, v, _ = _gpu(*_inputs(case, dtype))
    k2, v2 = _gpu(*_round2_kv(case, dtype))
    acc, m, l = _state(case.b, case.sq, case.n, case.d)
    ext.attn_fwd_accum(q, k2, v2, _scale(case), False, acc, m, l, False)
    ext.attn_fwd_accum(q, k, v, _scale(case), True, acc, m, l, True)
    o, lse = ext.attn_fwd_finalize(acc, m, l, dtype)
    _check("carry-causal", case, dtype, {"o": o, "lse": lse},
           _named(_carry_ref(case, dtype)))


def _shifted_state(case, dtype):
    """(acc, m, l) after a fresh causal round on (k, v) and the shifted
    causal carry-in round on round2_kv (tile_window's striped later-rank
    window)."""
    ext = _ext()
    q, k, v, _ = _gpu(*_inputs(case, dtype))
    k2, v2 = _gpu(*_round2_kv(case, dtype))
    acc, m, l = _state(case.b, case.sq, case.n, case.d)
    ext.attn_fwd_accum(q, k, v, _scale(case), True, acc, m, l, False)
    ext.attn_fwd_accum(q[:, 1:], k2[:, :-1], v2[:, :-1], _scale(case), True,
                       acc[:, 1:], m[:, :, 1:], l[:, :, 1:], True)
    return acc, m, l


@BY_DTYPE
@SHIFT_CASES
def test_fwd_carry_in_shifted(case, dtype):
    o, lse = _ext().attn_fwd_finalize(*_shifted_state(case, dtype), dtype)
    _check("carry-shifted", case, dtype, {"o": o, "lse": lse},
           _named(_shifted_ref(case, dtype)))


@pytest.mark.parametrize("which", ["below", "above"])
@BY_DTYPE
@pytest.mark.parametrize("case", bi.DOMINATED_CASES, ids=_id)
def test_fwd_carry_in_dominated(case, dtype, which):
    """The exp2-domain rescale of carried state at its ends: a causal
    carry-in round whose every score is 30 or more below the carried max
    (the result is round 1, to within the gate) or above it (the carried
    acc and l must vanish without leaving inf or nan behind)."""
    ext = _ext()
    q, k, v, _ = _gpu(*_inputs(case, dtype))
    k2, v2 = _gpu(*_dominated_kv(case, dtype, which))
    acc, m, l = _state(case.b, case.sq, case.n, case.d)
    ext.attn_fwd_accum(q, k, v, _scale(case), True, acc, m, l, False)
    ext.attn_fwd_accum(q, k2, v2, _scale(case), True, acc, m, l, True)
    o, lse = ext.attn_fwd_finalize(acc, m, l, dtype)
    for name, t in (("acc", acc), ("m", m), ("l", l), ("o", o), ("lse", lse)):
        assert bool(torch.isfinite(t).all()), name
    _check(f"carry-dominated-{which}", case, dtype, {"o": o, "lse": lse},
           _named(_dominated_ref(case, dtype, which)))
    if which == "below":
        _check("carry-dominated-below-vs-round1", case, dtype,
               {"o": o, "lse": lse}, _named(_fwd_ref(case, dtype)))


@FWD_ALT_KNOBS
@BY_DTYPE
@KNOB_CASES
def test_fwd_knobs_vs_oracle(knobs, case, dtype, monkeypatch):
    """Every env-selectable forward variant against the oracle, stateless
    and carry-in (test_gpu_parity.py compares them with the default
    variant only, on randn)."""
    for key, val in knobs.items():
        monkeypatch.setenv(key, val)
    tag = "+".join(f"{k[3:]}={v}" for k, v in knobs.items())
    _check(f"fwd[{tag}]", case, dtype, _stateless(case, dtype),
           _named(_fwd_ref(case, dtype)))
    _check(f"carry[{tag}]", case, dtype, _carry_in(case, dtype),
           _named(_carry_ref(case, dtype)))


# ---- backward

def _bwd(case, dtype, det):
    ext = _ext()
    q, k, v, do = _gpu(*_inputs(case, dtype))
    o, lse = ext.attn_fwd(q, k, v, _scale(case), case.causal)
    delta = ext.attn_bwd_preprocess(o.to(dtype), do)
    dq, dk, dv = ext.attn_bwd(do, q, k, v, delta, lse, _scale(case),
                              case.causal, det)
    assert dk.shape == k.shape and dv.shape == v.shape and dq.shape == q.shape
    return {"dq": dq, "dk": dk, "dv": dv}


def _named_grads(g):
    return dict(zip(("dq", "dk", "dv"), g))


# `deterministic` is part of the binding's contract, so both values are
# run; today's launcher ignores it (every default-plan kernel is
# deterministic by construction, attn_bwd.hip's bahip_attn_bwd_gqa), so
# the two ids run the same kernels until a plan honours the flag.
BY_DET = pytest.mark.parametrize("det", [False, True],
                                 ids=["atomic-ok", "det"])


@BY_DET
@BY_DTYPE
@CASES
def test_bwd_default_plan(case, dtype, det):
    _check("bwd", case, dtype, _bwd(case, dtype, det),
           _named_grads(_bwd_ref(case, dtype)))


@BY_DET
@BY_DTYPE
@SHIFT_CASES
def test_bwd_accum_under_merged_lse(case, dtype, det):
    """The backward as the ring calls it: lse and delta belong to the
    merged two-round forward of test_fwd_carry_in_shifted, not to the tile
    being differentiated, so a tile's P is a fragment of a row; both
    rounds' tiles accumulate into one dq, the second through the shifted
    views delta[:, :, 1:], lse[:, :, 1:], dq[:, 1:] and dk2/dv2[:, :-1]."""
    ext = _ext()
    q, k, v, do = _gpu(*_inputs(case, dtype))
    k2, v2 = _gpu(*_round2_kv(case, dtype))
    o, lse = ext.attn_fwd_finalize(*_shifted_state(case, dtype), dtype)
    delta = ext.attn_bwd_preprocess(o, do)
    zeros = lambda t: torch.zeros(t.shape, dtype=torch.float32, device="cuda")
    dq, dk, dv, dk2, dv2 = zeros(q), zeros(k), zeros(v), zeros(k2), zeros(v2)
    sc = _scale(case)
    ext.attn_bwd_accum(do, q, k, v, delta, lse, sc, True, det, dq, dk, dv)
    ext.attn_bwd_accum(do[:, 1:], q[:, 1:], k2[:, :-1], v2[:, :-1],
                       delta[:, :, 1:], lse[:, :, 1:], sc, True, det,
                       dq[:, 1:], dk2[:, :-1], dv2[:, :-1])
    names = ("dq", "dk", "dv", "dk2", "dv2")
    _check("bwd-merged-lse", case, dtype,
           dict(zip(names, (dq, dk, dv, dk2, dv2))),
           dict(zip(names, _merged_bwd_ref(case, dtype))))


# (knob, value, needs equal heads): the experiment plans of bwd_plans.h.
# The bwd_dkq_kernel plans are equal-heads only and run on the N = Nk cases
# (tests/test_gpu_gqa.py pins that they reject the others).
BWD_KNOBS = [("BA_BWD_FUSED", "1", True), ("BA_BWD_FUSED", "2", True),
             ("BA_BWD_DK_FLIP", "1", True), ("BA_DQ_PIPE", "1", False)]
BWD_KNOB_CASES = [(k, v, c) for k, v, eq in BWD_KNOBS for c in bi.KNOB_CASES
                  if not eq or c.n == c.nk]


@BY_DTYPE
@pytest.mark.parametrize(
    "knob,value,case", BWD_KNOB_CASES,
    ids=[f"{k[3:]}={v}-{_id(c)}" for k, v, c in BWD_KNOB_CASES])
def test_bwd_knobs_vs_oracle(knob, value, case, dtype, monkeypatch):
    """The backward experiment plans against the oracle (test_gpu_parity.py
    compares them with the default plan only, on randn)."""
    monkeypatch.setenv(knob, value)
    _check(f"bwd[{knob[3:]}={value}]", case, dtype, _bwd(case, dtype, False),
           _named_grads(_bwd_ref(case, dtype)))


# ---- strided views into poisoned parents

POISON_CASES = pytest.mark.parametrize(
    "case",
    [c for c in bi.CASES
     if c.family == "seam_weighted" and (c.n, c.nk) == (4, 2)
     and (c.sq, c.sk) in ((328, 328), (96, 320), (40, 33))],
    ids=_id)


class _Poisoned:
    """boundary_inputs.poisoned_parent on the GPU: `.v[name]` input views,
    `.out[name]` output views, and the untouched-outside check."""

    def __init__(self, q, k, v, do):
        self.cpu = bi.poisoned_parent(q, k, v, do)
        self.parents = {n: t.cuda() for n, t in self.cpu.parents.items()}
        self.out_parents = {n: t.cuda()
                            for n, t in self.cpu.out_parents.items()}
        self.v = {n: bi.view_of(self.parents[n], self.cpu.views[n],
                                self.cpu.parents[n]) for n in self.parents}
        self.out = {n: self._out_view(self.out_parents[n], n)
                    for n in self.out_parents}
        for name, t in self.v.items():
            assert not t.is_contiguous()
            assert torch.equal(t.cpu(), self.cpu.views[name])

    def _out_view(self, parent, name):
        return bi.view_of(parent, self.cpu.out_views[name],
                          self.cpu.out_parents[name])

    def assert_outside_untouched(self, names):
        for name in names:
            chk = self.out_parents[name].clone()
            self._out_view(chk, name).fill_(bi.SENTINEL)
            assert torch.equal(chk, torch.full_like(chk, bi.SENTINEL)), (
                f"{name}: written outside its view")


@BY_DTYPE
@POISON_CASES
def test_poisoned_parent_fwd_and_carry_in(case, dtype):
    """Nothing outside the q/k/v views is read (a leaked poison K row wins
    every softmax, a leaked V row is 1e4) and nothing outside the acc/m/l
    views is written."""
    ext = _ext()
    P = _Poisoned(*_inputs(case, dtype))
    q, k, v = P.v["q"], P.v["k"], P.v["v"]
    o, lse = ext.attn_fwd(q, k, v, _scale(case), case.causal)
    _check("poison-fwd", case, dtype, {"o": o, "lse": lse},
           _named(_fwd_ref(case, dtype)))
    k2c, v2c = _round2_kv(case, dtype)
    P2 = _Poisoned(_inputs(case, dtype)[0], k2c, v2c, _inputs(case, dtype)[3])
    acc, m, l = P.out["acc"], P.out["m"], P.out["l"]
    ext.attn_fwd_accum(q, k, v, _scale(case), case.causal, acc, m, l, False)
    ext.attn_fwd_accum(q, P2.v["k"], P2.v["v"], _scale(case), False, acc, m,
                       l, True)
    P.assert_outside_untouched(("acc", "m", "l"))
    o_c, lse_c = ext.attn_fwd_finalize(acc.contiguous(), m.contiguous(),
                                       l.contiguous(), dtype)
    _check("poison-carry", case, dtype, {"o": o_c, "lse": lse_c},
           _named(_carry_ref(case, dtype)))


@BY_DET
@BY_DTYPE
@POISON_CASES
def test_poisoned_parent_bwd_accum(case, dtype, det):
    """attn_bwd_accum on views: parity inside the dq/dk/dv views (zeroed
    first: the call accumulates), the sentinel everywhere outside them."""
    ext = _ext()
    P = _Poisoned(*_inputs(case, dtype))
    q, k, v, do = P.v["q"], P.v["k"], P.v["v"], P.v["do"]
    o, lse = ext.attn_fwd(q, k, v, _scale(case), case.causal)
    delta = ext.attn_bwd_preprocess(o.to(dtype), do)
    grads = {n: P.out[n] for n in ("dq", "dk", "dv")}
    for g in grads.values():
        g.zero_()
    ext.attn_bwd_accum(do, q, k, v, delta, lse, _scale(case), case.causal,
                       det, grads["dq"], grads["dk"], grads["dv"])
    P.assert_outside_untouched(("dq", "dk", "dv"))
    _check("poison-bwd", case, dtype, grads,
           _named_grads(_bwd_ref(case, dtype)))
