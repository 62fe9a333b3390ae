"""CPU proof for tests/test_gpu_ring_rounds.py: the replay is right, and
on its cases the parity gates see an error confined to one ring seam.

(a) ``ring_rounds.replay_ring`` with the oracle tile provider on fp32
    inputs equals full-sequence eager attention, at W = 1..4, both
    layouts, causal and not, equal and grouped heads.

(b) Sensitivity, in the manner of tests/test_gate_sensitivity_cpu.py and
    with its CAUGHT / CLEAN: on every case of ``ring_rounds.CASES`` and
    both dtypes' gates (``boundary_refs.gates``), the rounding emulation of
    the unmutated full-sequence math scores <= CLEAN on every output, and
    every mutant below scores >= CAUGHT on at least one output in at least
    one case of its layout.  A mutant imitates a kernel (or launcher) that
    is one pair or one row wrong in a form only the ring's rounds produce:

    window mutants — the full-sequence math under the [S, S] allow-mask
    the W x W tiles compose to (``ring_rounds.allow_mask``; with the
    shipped ``tile_window`` it is tril, asserted), with one rank relation's
    window changed:
      striped  later_unshifted    a later rank's tile run unshifted: the
                                  same-index key leaks
      striped  earlier_shifted    an earlier rank's tile run shifted: the
                                  boundary key is dropped
      striped  earlier_strict     ... or run with j < i
      zigzag   earlier_kv_short   kv window half - 1: the tail key dropped
      zigzag   earlier_kv_long    kv window half + 1: one key leaked
      zigzag   later_q_late       q window from half + 1: the second
                                  half's first row never sees later chunks
      zigzag   later_q_early      q window from half - 1: a first-half row
                                  sees them
    replay mutants — ``replay_ring`` with an oracle provider that is wrong
    in what the mask cannot express:
      row_offset+1 / -1           the right rows computed, merged into the
                                  neighbouring state rows
      carry_ignored               round 2 overwrites the state's rows
                                  instead of merging into them
      dkv_target+1                the dk/dv[:, kw] view taken one row late
      dq_target-1                 the dq[:, qw] view taken one row early

``summary_table()`` gives the figures recorded in
profiles/gate_sensitivity/README.md.
"""

import dataclasses
import functools

import pytest
import torch

import oracle

from burst_attn_amd.interface import tile_window

from . import mutant_oracle as mo
from . import ring_rounds as rr
from .boundary_inputs import dtype_name as _dt
from .boundary_refs import gates
from .gqa_cpu_provider import (GqaOracleTileProvider, expand_kv,
                               gqa_full_reference)
from .test_gate_sensitivity_cpu import CAUGHT, CLEAN

DTYPES = [torch.float16, torch.bfloat16]
OUTPUTS = ("o", "lse", "dq", "dk", "dv")

# (layout, mutant, dtype name) -> best ratio over the layout's cases, for a
# mutant that reaches CAUGHT on none of them.  At most 2 may be listed.
NOT_SEPARABLE = {}


# ---- (a) the replay is right

@pytest.mark.parametrize("n,nk", [(2, 2), (4, 2)])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("layout", ["zigzag", "striped"])
@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_replay_equals_full_sequence(W, layout, causal, n, nk):
    b, s_local, d = 2, 10, 16
    S = W * s_local
    g = torch.Generator().manual_seed(31 * W + n)
    q, do = (torch.randn(b, S, n, d, generator=g) for _ in range(2))
    k, v = (torch.randn(b, S, nk, d, generator=g) for _ in range(2))
    scale = d ** -0.5
    P = GqaOracleTileProvider()
    o, lse, dq, dk, dv = rr.replay_ring(P, q, k, v, do, W, scale, causal,
                                        layout)
    assert set(P.fwd_kv_heads) == {(nk, nk)} == set(P.bwd_kv_heads)
    o_r, dq_r, dk_r, dv_r = gqa_full_reference(q, k, v, do, scale, causal)
    lse_r = mo.forward(q, k, v, scale, mo.base_spec(
        mo.Ctx(b, S, S, n, nk, causal)))[1]
    tol = dict(rtol=1e-4, atol=1e-4)
    for out, ref in ((o, o_r), (lse, lse_r), (dq, dq_r), (dk, dk_r),
                     (dv, dv_r)):
        torch.testing.assert_close(out, ref, **tol)


# ---- (b) window mutants: tile_window with one rank relation changed

_ALL = slice(None)


def _window_mutant(layout, later, make):
    """tile_window, except that on `layout`, causal, for b > a (`later`)
    or b < a the window is make(half)."""
    def window(lay, a, b, causal, s_local):
        if lay == layout and causal and a != b and (b > a) == later:
            return make(s_local // 2)
        return tile_window(lay, a, b, causal, s_local)
    return window


WINDOW_MUTANTS = {
    "striped": {
        "later_unshifted": _window_mutant(
            "striped", True, lambda h: (_ALL, _ALL, True)),
        "earlier_shifted": _window_mutant(
            "striped", False, lambda h: (slice(1, None), slice(None, -1),
                                         True)),
        "earlier_strict": _window_mutant(
            "striped", False, lambda h: (_ALL, _ALL, "strict")),
    },
    "zigzag": {
        "earlier_kv_short": _window_mutant(
            "zigzag", False, lambda h: (_ALL, slice(None, h - 1), False)),
        "earlier_kv_long": _window_mutant(
            "zigzag", False, lambda h: (_ALL, slice(None, h + 1), False)),
        "later_q_late": _window_mutant(
            "zigzag", True, lambda h: (slice(h + 1, None), _ALL, False)),
        "later_q_early": _window_mutant(
            "zigzag", True, lambda h: (slice(h - 1, None), _ALL, False)),
    },
}


@functools.lru_cache(maxsize=None)
def _allow(layout, W, s_local, mutant=None):
    window = WINDOW_MUTANTS[layout][mutant] if mutant else tile_window
    return rr.allow_mask(layout, W, s_local, window)


@pytest.mark.parametrize("layout,W", sorted({(c.layout, c.W)
                                             for c in rr.CASES if c.causal}))
def test_shipped_windows_compose_to_tril(layout, W):
    S = W * rr.S_LOCAL
    assert torch.equal(_allow(layout, W, rr.S_LOCAL),
                       torch.ones(S, S, dtype=torch.bool).tril())
    for name in WINDOW_MUTANTS[layout]:
        bad = _allow(layout, W, rr.S_LOCAL, name)
        assert not torch.equal(bad, _allow(layout, W, rr.S_LOCAL)), name
        assert bool(bad.any(dim=1).all()), name


# ---- (b) replay mutants: an oracle provider that is wrong in one form

REPLAY_MUTANTS = ("row_offset+1", "row_offset-1", "carry_ignored",
                  "dkv_target+1", "dq_target-1")


def _row_shifted(view, rows):
    """The same-shaped view `rows` rows further into its parent."""
    return view.as_strided(view.shape, view.stride(),
                           view.storage_offset() + rows * view.stride(1))


class FaultyProvider(GqaOracleTileProvider):
    """The oracle provider with one of REPLAY_MUTANTS.  The shifted views
    stay inside their parents: a view is shifted only towards rows its
    window leaves free (the views of windowed rounds are not contiguous at
    b = 2, the full ones are)."""

    def __init__(self, fault):
        super().__init__()
        assert fault in REPLAY_MUTANTS
        self.fault = fault
        self.carry_calls = 0

    def fwd_accum(self, state, q, k, v, scale, causal, row_offset=0):
        if state is None:
            self.carry_calls = 0
            return super().fwd_accum(state, q, k, v, scale, causal, 0)
        self.carry_calls += 1
        n, sq = q.shape[2], q.shape[1]
        if self.fault == "carry_ignored" and self.carry_calls == 1:
            o_i, lse_i = oracle.tile_fwd(q, expand_kv(k, n), expand_kv(v, n),
                                         scale, causal)
            sl = slice(row_offset, row_offset + sq)
            state[0][:, sl] = o_i
            state[1][:, sl] = lse_i.transpose(-2, -1).unsqueeze(-1)
            return state
        if self.fault.startswith("row_offset") and row_offset > 0:
            if self.fault.endswith("-1"):
                return super().fwd_accum(state, q, k, v, scale, causal,
                                         row_offset - 1)
            # one row late: the last row has no state row to land in
            o_i, lse_i = oracle.tile_fwd(q, expand_kv(k, n), expand_kv(v, n),
                                         scale, causal)
            o, lse = state
            sl = slice(row_offset + 1, row_offset + sq)
            o[:, sl], lse[:, sl] = oracle.scale_out_lse(
                o[:, sl], lse[:, sl], o_i[:, :-1], lse_i[:, :, :-1])
            return state
        return super().fwd_accum(state, q, k, v, scale, causal, row_offset)

    def bwd_accum(self, do, q, k, v, delta, lse, scale, causal, deterministic,
                  dq, dk, dv):
        if (self.fault == "dkv_target+1" and not dk.is_contiguous()
                and dk.storage_offset() == 0):
            dk, dv = _row_shifted(dk, 1), _row_shifted(dv, 1)
        if self.fault == "dq_target-1" and dq.storage_offset() > 0:
            dq = _row_shifted(dq, -1)
        super().bwd_accum(do, q, k, v, delta, lse, scale, causal,
                          deterministic, dq, dk, dv)


def mutants_of(case):
    if not case.causal:
        return ("carry_ignored",)
    return tuple(WINDOW_MUTANTS[case.layout]) + REPLAY_MUTANTS


# ---- scoring

def _ratios(outs, refs, dtype, g):
    gt = gates(dtype, g)
    return {name: mo.gate_ratio(outs[name], refs[name], **gt[name])
            for name in outs}


@functools.lru_cache(maxsize=None)
def evaluate(case, dtype):
    """{"emu": {output: ratio}, mutant: {output: ratio}} of one case
    against the fp32 full-sequence math on the same (rounded) inputs."""
    q, k, v, do = rr.make_inputs(case, dtype)
    scale, grp = rr.scale_of(case), case.n // case.nk
    S = case.W * case.s_local
    base = mo.base_spec(mo.Ctx(case.b, S, S, case.n, case.nk, case.causal))
    if case.causal:
        base = dataclasses.replace(
            base, allow=_allow(case.layout, case.W, case.s_local))
    o, lse = mo.forward(q, k, v, scale, base)
    ref = dict(zip(OUTPUTS, (o, lse, *mo.backward(do, q, k, v, o, lse, scale,
                                                  base))))
    score = lambda outs: _ratios(dict(zip(OUTPUTS, outs)), ref, dtype, grp)

    o_e, lse_e = mo.forward(q, k, v, scale, base, round_dtype=dtype)
    out = {"emu": score((o_e, lse_e, *mo.backward(
        do, q, k, v, o_e, lse_e, scale, base, round_dtype=dtype)))}
    for name in mutants_of(case):
        if name in REPLAY_MUTANTS:
            got = rr.replay_ring(FaultyProvider(name), q, k, v, do, case.W,
                                 scale, case.causal, case.layout)
            out[name] = score(tuple(t.float() for t in got))
        else:
            spec = dataclasses.replace(
                base, allow=_allow(case.layout, case.W, case.s_local, name))
            o_m, lse_m = mo.forward(q, k, v, scale, spec)
            # the backward's window is wrong under the right forward
            out[name] = score((o_m, lse_m, *mo.backward(
                do, q, k, v, o, lse, scale, spec)))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("case", rr.CASES, ids=rr.case_id)
def test_rounding_emulation_passes(case, dtype):
    over = {k: r for k, r in evaluate(case, dtype)["emu"].items()
            if r > CLEAN}
    assert not over, over


def _best(layout, mutant, dtype):
    """A mutant's worst gate ratio per case of the layout it applies to."""
    return [max(evaluate(c, dtype)[mutant].values()) for c in rr.CASES
            if c.layout == layout and mutant in mutants_of(c)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("layout", ["zigzag", "striped"])
def test_mutants_rejected(layout, dtype):
    missed = {}
    for mutant in tuple(WINDOW_MUTANTS[layout]) + REPLAY_MUTANTS:
        if (layout, mutant, _dt(dtype)) in NOT_SEPARABLE:
            continue
        best = max(_best(layout, mutant, dtype))
        if best < CAUGHT:
            missed[mutant] = best
    assert not missed, missed


def test_not_separable_budget():
    assert len(NOT_SEPARABLE) <= 2
    for (layout, mutant, dt), _ in NOT_SEPARABLE.items():
        dtype = next(d for d in DTYPES if _dt(d) == dt)
        assert max(_best(layout, mutant, dtype)) < CAUGHT, (
            "separable after all: unlist it")


def summary_table():
    """Rows (layout, mutant or "emulation", dtype, min, max over the
    layout's cases of the worst output's ratio)."""
    rows = []
    for layout in ("zigzag", "striped"):
        for dtype in DTYPES:
            emu = [max(evaluate(c, dtype)["emu"].values()) for c in rr.CASES
                   if c.layout == layout]
            rows.append((layout, "emulation", _dt(dtype), min(emu), max(emu)))
            for mutant in tuple(WINDOW_MUTANTS[layout]) + REPLAY_MUTANTS:
                r = _best(layout, mutant, dtype)
                rows.append((layout, mutant, _dt(dtype), min(r), max(r)))
    return rows
