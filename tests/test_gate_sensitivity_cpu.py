"""CPU proof that the parity gates bite on the boundary input families.

The GPU boundary tests (tests/test_gpu_boundary.py) hold the kernels to the
fixed gates of tests/test_gpu_parity.py on the input families of
tests/boundary_inputs.py.  This module shows, without a GPU, that on those
inputs and at those shapes the gates separate a one-predicate error from
legitimate low-precision rounding.  For every case of
``boundary_inputs.CASES`` and both dtypes' gates, with
ratio = max |err| / (atol + rtol |ref|) per asserted output:

(a) every applicable mutant of tests/mutant_oracle.py (the fp32 math with
    one kernel predicate off by one) scores >= 3 on at least one of the
    outputs its stage asserts ("fwd": o, lse of the stateless call;
    "carry": o, lse of the two-call carry-in form, scored as one softmax
    over [round-1 keys under the mutated mask | boundary_inputs.round2_kv
    unmasked]; "shift": o, lse of the striped ring's shifted carry-in
    form, causal cases with Sq >= 2, one softmax over [the keys under the
    causal mask | round2_kv[:-1] for rows 1.. under the causal mask of
    that (Sq-1, Sk-1) tile], the mutant in both tiles' predicates, each at
    its own shape, since both are calls of the same causal kernel; "bwd":
    dq, dk, dv with the forward left right);
(b) the rounding emulation of the unmutated math (P, dS and the o behind
    delta rounded to the input dtype) scores <= 0.5 on every output.

Both are asserted.  As one softmax the "carry" form does not depend on the
order of its two rounds, so it stands for test_fwd_carry_in (masked round
first) and test_fwd_carry_in_causal (masked round second, the striped
ring's order) alike.  The table lists, per (family, mutant, stage, dtype),
the mutant's score at the shape where it is caught least (minimum over the
applicable cases of its best output) and the emulation's worst score over
the family's cases; the last two columns are the same figures with plain
randn inputs at the same shapes, the control.  (The control's minimum is
mostly set by a large shape; mutants that touch the first rows, where a
row has a handful of keys, are caught with any input.)

family         mutant                 stage dtype    mutant emulation randn mut randn emu
seam_weighted  tail_exclusive         fwd   fp16      22.46      0.31      0.79      0.07
seam_weighted  tail_exclusive         carry fp16      17.53      0.05      0.39      0.05
seam_weighted  tail_exclusive         shift fp16      20.34      0.04      0.63      0.04
seam_weighted  tail_exclusive         bwd   fp16      34.14      0.31      0.46      0.07
seam_weighted  tail_inclusive         fwd   fp16      34.61      0.31      5.70      0.07
seam_weighted  tail_inclusive         carry fp16      47.09      0.05      3.12      0.05
seam_weighted  tail_inclusive         bwd   fp16      68.43      0.31      4.22      0.07
seam_weighted  strict_diag_ge32       fwd   fp16      73.46      0.31      7.12      0.07
seam_weighted  strict_diag_ge32       carry fp16      62.64      0.05      3.54      0.05
seam_weighted  strict_diag_ge32       shift fp16      63.36      0.04      3.59      0.04
seam_weighted  strict_diag_ge32       bwd   fp16      57.28      0.31      4.39      0.07
seam_weighted  superdiag_leak         fwd   fp16     156.99      0.31    176.89      0.07
seam_weighted  superdiag_leak         carry fp16     113.09      0.05      6.45      0.05
seam_weighted  superdiag_leak         shift fp16     127.88      0.04    156.99      0.04
seam_weighted  superdiag_leak         bwd   fp16     158.70      0.31    322.21      0.07
seam_weighted  full_subtile_early     fwd   fp16       4.28      0.31     13.54      0.07
seam_weighted  full_subtile_early     carry fp16       2.40      0.05      6.79      0.05   not separable at this gate
seam_weighted  full_subtile_early     shift fp16       3.63      0.04      8.84      0.04
seam_weighted  last_tile_skipped      fwd   fp16      33.91      0.31     29.72      0.07
seam_weighted  last_tile_skipped      carry fp16      26.78      0.05     10.98      0.05
seam_weighted  last_tile_skipped      shift fp16      30.71      0.04     17.24      0.04
seam_weighted  last_tile_skipped      bwd   fp16      28.09      0.31     15.40      0.07
seam_weighted  bwd_t0_late            bwd   fp16      63.68      0.31      6.18      0.07
seam_weighted  q_tail_twice           bwd   fp16      39.95      0.31      3.61      0.07
seam_weighted  head_map_mod           fwd   fp16     228.67      0.31     56.32      0.07
seam_weighted  head_map_mod           carry fp16     208.98      0.05     41.55      0.05
seam_weighted  head_map_mod           shift fp16     290.16      0.04    309.79      0.04
seam_weighted  head_map_mod           bwd   fp16     116.56      0.31     36.79      0.07
seam_weighted  batch1_reads_batch0_k  fwd   fp16      57.43      0.31     42.25      0.07
seam_weighted  batch1_reads_batch0_k  carry fp16      97.12      0.05     30.52      0.05
seam_weighted  batch1_reads_batch0_k  shift fp16     152.77      0.04    140.49      0.04
seam_weighted  batch1_reads_batch0_k  bwd   fp16      84.12      0.31     28.66      0.07
seam_weighted  tail_exclusive         fwd   bf16       4.45      0.39      0.16      0.08
seam_weighted  tail_exclusive         carry bf16       3.40      0.06      0.08      0.07
seam_weighted  tail_exclusive         shift bf16       3.95      0.06      0.13      0.07
seam_weighted  tail_exclusive         bwd   bf16       6.62      0.39      0.09      0.08
seam_weighted  tail_inclusive         fwd   bf16      14.36      0.39      1.10      0.08
seam_weighted  tail_inclusive         carry bf16      13.27      0.06      0.61      0.07
seam_weighted  tail_inclusive         bwd   bf16      13.47      0.39      0.84      0.08
seam_weighted  strict_diag_ge32       fwd   bf16      14.03      0.39      1.40      0.08
seam_weighted  strict_diag_ge32       carry bf16      12.08      0.06      0.70      0.07
seam_weighted  strict_diag_ge32       shift bf16      12.21      0.06      0.72      0.07
seam_weighted  strict_diag_ge32       bwd   bf16      10.81      0.39      0.87      0.08
seam_weighted  superdiag_leak         fwd   bf16      29.52      0.39     56.92      0.08
seam_weighted  superdiag_leak         carry bf16      21.09      0.06      1.27      0.07
seam_weighted  superdiag_leak         shift bf16      24.27      0.06     56.92      0.07
seam_weighted  superdiag_leak         bwd   bf16      31.33      0.39     64.90      0.08
seam_weighted  full_subtile_early     fwd   bf16       1.10      0.39      5.28      0.08   not separable at this gate
seam_weighted  full_subtile_early     carry bf16       0.78      0.06      2.51      0.07   not separable at this gate
seam_weighted  full_subtile_early     shift bf16       1.63      0.06      4.79      0.07      not separable at this gate
seam_weighted  last_tile_skipped      fwd   bf16       7.88      0.39     14.42      0.08
seam_weighted  last_tile_skipped      carry bf16       5.12      0.06      5.42      0.07
seam_weighted  last_tile_skipped      shift bf16       7.90      0.06     12.73      0.07
seam_weighted  last_tile_skipped      bwd   bf16       5.60      0.39      3.05      0.08
seam_weighted  bwd_t0_late            bwd   bf16      12.15      0.39      1.23      0.08
seam_weighted  q_tail_twice           bwd   bf16       7.97      0.39      0.72      0.08
seam_weighted  head_map_mod           fwd   bf16      51.13      0.39     12.33      0.08
seam_weighted  head_map_mod           carry bf16      45.86      0.06      8.47      0.07
seam_weighted  head_map_mod           shift bf16      93.61      0.06     70.42      0.07
seam_weighted  head_map_mod           bwd   bf16      22.26      0.39      7.26      0.08
seam_weighted  batch1_reads_batch0_k  fwd   bf16      44.50      0.39      9.78      0.08
seam_weighted  batch1_reads_batch0_k  carry bf16      41.03      0.06      7.30      0.07
seam_weighted  batch1_reads_batch0_k  shift bf16      78.01      0.06     51.31      0.07
seam_weighted  batch1_reads_batch0_k  bwd   bf16      15.38      0.39      5.69      0.08
diag_needle    tail_exclusive         fwd   fp16      57.91      0.18      0.79      0.07
diag_needle    tail_exclusive         carry fp16      41.44      0.03      0.39      0.02
diag_needle    tail_exclusive         shift fp16      41.40      0.03      0.63      0.04
diag_needle    tail_exclusive         bwd   fp16      24.82      0.18      0.46      0.07
diag_needle    strict_diag_ge32       fwd   fp16     124.28      0.18      7.12      0.07
diag_needle    strict_diag_ge32       carry fp16      88.72      0.03      3.54      0.02
diag_needle    strict_diag_ge32       shift fp16      89.31      0.03      3.59      0.04
diag_needle    strict_diag_ge32       bwd   fp16      39.02      0.18      4.39      0.07
diag_needle    superdiag_leak         fwd   fp16     396.22      0.18    176.89      0.07
diag_needle    superdiag_leak         carry fp16     382.41      0.03      6.45      0.02
diag_needle    superdiag_leak         shift fp16     390.05      0.03    156.99      0.04
diag_needle    superdiag_leak         bwd   fp16   63885.03      0.18    322.21      0.07
diag_needle    full_subtile_early     fwd   fp16     356.27      0.18     13.54      0.07
diag_needle    full_subtile_early     carry fp16     354.28      0.03      6.79      0.02
diag_needle    full_subtile_early     shift fp16     354.36      0.03      8.84      0.04
diag_needle    last_tile_skipped      fwd   fp16     174.47      0.18     29.72      0.07
diag_needle    last_tile_skipped      carry fp16     164.12      0.03     10.98      0.02
diag_needle    last_tile_skipped      shift fp16     167.88      0.03     17.24      0.04
diag_needle    last_tile_skipped      bwd   fp16      74.27      0.18     15.40      0.07
diag_needle    bwd_t0_late            bwd   fp16      48.43      0.18      6.18      0.07
diag_needle    q_tail_twice           bwd   fp16      22.39      0.18      3.61      0.07
diag_needle    head_map_mod           fwd   fp16     290.16      0.18    302.15      0.07
diag_needle    head_map_mod           carry fp16     178.86      0.03     59.75      0.02
diag_needle    head_map_mod           shift fp16     290.16      0.03    309.79      0.04
diag_needle    head_map_mod           bwd   fp16      65.58      0.18    490.48      0.07
diag_needle    batch1_reads_batch0_k  fwd   fp16      21.51      0.18     42.25      0.07
diag_needle    batch1_reads_batch0_k  carry fp16     159.11      0.03     42.33      0.02
diag_needle    batch1_reads_batch0_k  shift fp16     196.36      0.03    140.49      0.04
diag_needle    batch1_reads_batch0_k  bwd   fp16      35.12      0.18     46.56      0.07
diag_needle    tail_exclusive         fwd   bf16      10.48      0.30      0.16      0.08
diag_needle    tail_exclusive         carry bf16       7.65      0.05      0.08      0.06
diag_needle    tail_exclusive         shift bf16       7.64      0.05      0.13      0.07
diag_needle    tail_exclusive         bwd   bf16       4.85      0.30      0.09      0.08
diag_needle    strict_diag_ge32       fwd   bf16      23.55      0.30      1.40      0.08
diag_needle    strict_diag_ge32       carry bf16      16.25      0.05      0.70      0.06
diag_needle    strict_diag_ge32       shift bf16      16.20      0.05      0.72      0.07
diag_needle    strict_diag_ge32       bwd   bf16       7.48      0.30      0.87      0.08
diag_needle    superdiag_leak         fwd   bf16     237.73      0.30     56.92      0.08
diag_needle    superdiag_leak         carry bf16     195.24      0.05      1.27      0.06
diag_needle    superdiag_leak         shift bf16     227.76      0.05     56.92      0.07
diag_needle    superdiag_leak         bwd   bf16   12624.91      0.30     64.90      0.08
diag_needle    full_subtile_early     fwd   bf16     236.31      0.30      5.28      0.08
diag_needle    full_subtile_early     carry bf16     225.76      0.05      2.51      0.06
diag_needle    full_subtile_early     shift bf16     226.43      0.05      4.79      0.07
diag_needle    last_tile_skipped      fwd   bf16      99.21      0.30     14.42      0.08
diag_needle    last_tile_skipped      carry bf16      79.72      0.05      5.42      0.06
diag_needle    last_tile_skipped      shift bf16      87.78      0.05     12.73      0.07
diag_needle    last_tile_skipped      bwd   bf16      13.88      0.30      3.05      0.08
diag_needle    bwd_t0_late            bwd   bf16       9.25      0.30      1.23      0.08
diag_needle    q_tail_twice           bwd   bf16       4.39      0.30      0.72      0.08
diag_needle    head_map_mod           fwd   bf16     135.01      0.30     83.44      0.08
diag_needle    head_map_mod           carry bf16      77.07      0.05     13.66      0.06
diag_needle    head_map_mod           shift bf16     152.04      0.05     70.42      0.07
diag_needle    head_map_mod           bwd   bf16      12.78      0.30     97.93      0.08
diag_needle    batch1_reads_batch0_k  fwd   bf16      21.65      0.30     42.23      0.08
diag_needle    batch1_reads_batch0_k  carry bf16      52.14      0.05     10.59      0.06
diag_needle    batch1_reads_batch0_k  shift bf16     124.17      0.05     51.31      0.07
diag_needle    batch1_reads_batch0_k  bwd   bf16       6.60      0.30      8.63      0.08

One mutant is not separable at this gate on seam_weighted, in both dtypes:
a diagonal 32x32 subtile taken as full leaks only ordinary keys there (the
family's weighted keys sit on the seams, none strictly inside that subtile
above the diagonal), about 1% of a row's mass and half that once the
carry-in form's second round has added Sk more keys.  That is 1.10 (fwd)
and 0.78 (carry) bf16 gates against 0.39 and 0.06 for the emulation, 1.63
in the shifted form, and 2.40 fp16 gates in the carry form (4.28 stateless
and 3.63 shifted, which are caught).  The cases stay in the suite;
the diag_needle family rejects the same mutant at 226 or more in every
stage and dtype.
"""

import dataclasses
import functools
import math

import pytest
import torch

from . import mutant_oracle as mo
from .boundary_inputs import CASES, case_id as _id, dtype_name as _dt
from .boundary_refs import gates, inputs, round2_kv

DTYPES = [torch.float16, torch.bfloat16]
CAUGHT = 3.0   # condition (a): a mutant's worst gate ratio is at least this
CLEAN = 0.5    # condition (b): the rounding emulation's is at most this

# (family, mutant, dtype name) pairs "not separable at this gate" and the
# stages in which they are not; see the module docstring.  At most 2 pairs
# may be listed.
NOT_SEPARABLE = {
    ("seam_weighted", "full_subtile_early", "bf16"): ("fwd", "carry",
                                                     "shift"),
    ("seam_weighted", "full_subtile_early", "fp16"): ("carry",),
}
# evaluate()'s rounding-emulation keys (emu_shift: causal cases, Sq >= 2)
EMU = ("emu", "emu_carry", "emu_shift")
STAGES = ("fwd", "carry", "shift", "bwd")
_EMU_OF = {"carry": "emu_carry", "shift": "emu_shift"}


def _ratios(outs, refs, dtype, g):
    gt = gates(dtype, g)
    return {name: mo.gate_ratio(outs[name], refs[name], **gt[name])
            for name in outs}


def _ctx(case):
    return mo.Ctx(case.b, case.sq, case.sk, case.n, case.nk, case.causal)


@functools.lru_cache(maxsize=None)
def evaluate(case, dtype, randn=False):
    """{"emu": {output: ratio}, (mutant, stage): {output: ratio}} for one
    case: the fp32 math against itself with one predicate changed, and
    against its rounding emulation.  randn=True swaps the family's inputs
    for plain randn ones (the control)."""
    if randn:
        g = torch.Generator().manual_seed(7)
        mk = lambda s, h: torch.randn(case.b, s, h, case.d,
                                      generator=g).to(dtype)
        q, k, v, do = (mk(case.sq, case.n), mk(case.sk, case.nk),
                       mk(case.sk, case.nk), mk(case.sq, case.n))
    else:
        q, k, v, do = inputs(case, dtype)
    scale = 1.0 / math.sqrt(case.d)
    ctx = _ctx(case)
    grp = case.n // case.nk
    base = mo.base_spec(ctx)
    o, lse = mo.forward(q, k, v, scale, base)
    dq, dk, dv = mo.backward(do, q, k, v, o, lse, scale, base)
    ref_f = {"o": o, "lse": lse}
    ref_b = {"dq": dq, "dk": dk, "dv": dv}

    out = {}
    o_e, lse_e = mo.forward(q, k, v, scale, base, round_dtype=dtype)
    g_e = mo.backward(do, q, k, v, o_e, lse_e, scale, base, round_dtype=dtype)
    out["emu"] = {
        **_ratios({"o": o_e, "lse": lse_e}, ref_f, dtype, grp),
        **_ratios(dict(zip(("dq", "dk", "dv"), g_e)), ref_b, dtype, grp)}
    # the carry-in form: round 1 under the case's mask, then Sk more keys
    # unmasked (the GPU tests' second call), scored as one softmax over
    # [round-1 keys | round-2 keys]; a mutant changes round 1's predicate
    if randn:
        k2, v2 = mk(case.sk, case.nk), mk(case.sk, case.nk)
    else:
        k2, v2 = round2_kv(case, dtype)

    def carry(spec, round_dtype=None):
        tail = [k[:, -1:]] if spec.dup_tail else []
        vtail = [v[:, -1:]] if spec.dup_tail else []
        both = dataclasses.replace(
            spec, dup_tail=False,
            allow=torch.cat([spec.allow, torch.ones(
                case.sq, case.sk, dtype=torch.bool)], 1),
            kv_weight=torch.ones(1))
        o_c, lse_c = mo.forward(q, torch.cat([k, *tail, k2], 1),
                                torch.cat([v, *vtail, v2], 1), scale, both,
                                round_dtype)
        return {"o": o_c, "lse": lse_c}

    ref_c = carry(base)
    out["emu_carry"] = _ratios(carry(base, dtype), ref_c, dtype, grp)

    # the shifted carry-in form (test_fwd_carry_in_shifted): round 1 on
    # (k, v) under the causal mask, then rows 1.. against k2[:-1] under the
    # causal mask of that (Sq-1, Sk-1) tile.  Both rounds are the same
    # causal kernel, so a mutant changes the predicate of both tiles, each
    # at its own shape.
    shifted_form = case.causal and case.sq >= 2
    if shifted_form:
        ctx2 = ctx._replace(sq=case.sq - 1, sk=case.sk - 1)

        def shifted(spec1, spec2, round_dtype=None):
            allow = torch.zeros(case.sq, 2 * case.sk - 1, dtype=torch.bool)
            allow[:, :case.sk] = spec1.allow
            allow[1:, case.sk:] = spec2.allow
            both = dataclasses.replace(spec1, allow=allow,
                                       kv_weight=torch.ones(1))
            o_s, lse_s = mo.forward(q, torch.cat([k, k2[:, :-1]], 1),
                                    torch.cat([v, v2[:, :-1]], 1), scale,
                                    both, round_dtype)
            return {"o": o_s, "lse": lse_s}

        base2 = mo.base_spec(ctx2)
        ref_s = shifted(base, base2)
        out["emu_shift"] = _ratios(shifted(base, base2, dtype), ref_s, dtype,
                                   grp)
    for mut in mo.MUTANTS:
        if shifted_form and "fwd" in mut.stages:
            spec1, spec2 = mo.mutate(mut, ctx), mo.mutate(mut, ctx2)
            if spec1 is not None or spec2 is not None:
                out[mut.name, "shift"] = _ratios(
                    shifted(spec1 or base, spec2 or base2), ref_s, dtype, grp)
        spec = mo.mutate(mut, ctx)
        if spec is None:
            continue
        if "fwd" in mut.stages:
            o_m, lse_m = mo.forward(q, k, v, scale, spec)
            out[mut.name, "fwd"] = _ratios({"o": o_m, "lse": lse_m}, ref_f,
                                           dtype, grp)
            out[mut.name, "carry"] = _ratios(carry(spec), ref_c, dtype, grp)
        if "bwd" in mut.stages:
            # the forward is right; the backward's predicate is wrong
            g_m = mo.backward(do, q, k, v, o, lse, scale, spec)
            out[mut.name, "bwd"] = _ratios(
                dict(zip(("dq", "dk", "dv"), g_m)), ref_b, dtype, grp)
    # a mutant that moves no output by a thousandth of its gate is no error
    # at this shape (tail_inclusive's backward at Sk = 1: the duplicate of
    # the only key has dS = 0 up to fp32 roundoff and no dk/dv row of its
    # own)
    return {k: r for k, r in out.items()
            if k in EMU or max(r.values()) > 1e-3}


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_mutants_rejected(case, dtype):
    """(a) every applicable mutant fails at least one asserted output by 3x
    its gate."""
    res = evaluate(case, dtype)
    missed = []
    for key, ratios in res.items():
        if key in EMU:
            continue
        if key[1] in NOT_SEPARABLE.get((case.family, key[0], _dt(dtype)), ()):
            continue
        if max(ratios.values()) < CAUGHT:
            missed.append((key, ratios))
    assert not missed, missed


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_rounding_emulation_passes(case, dtype):
    """(b) P, dS and o rounded to the input dtype stay under half of every
    gate."""
    res = evaluate(case, dtype)
    over = {(e, k): r for e in EMU if e in res for k, r in res[e].items()
            if r > CLEAN}
    assert not over, over


def test_every_mutant_applies_somewhere():
    """A mutant whose seam lies in none of the shapes would prove nothing."""
    for family in ("seam_weighted", "diag_needle"):
        seen = set()
        for case in CASES:
            if case.family == family:
                seen |= {k for k in evaluate(case, torch.bfloat16)
                         if k not in EMU}
        want = {(m.name, s) for m in mo.MUTANTS for s in _stages(m)}
        # the shifted form is causal, and so is diag_needle: no key past
        # the tail
        want -= {("tail_inclusive", "shift")}
        if family == "diag_needle":
            want -= {("tail_inclusive", s) for s in STAGES}
        assert seen == want, want ^ seen


def _stages(mut):
    """A forward predicate serves the stateless and the carry-in calls."""
    return [s for s in STAGES
            if (s if s not in _EMU_OF else "fwd") in mut.stages]


def test_not_separable_budget():
    assert len(NOT_SEPARABLE) <= 2


def test_docstring_table_is_current():
    """The table above is what this module computes (family columns)."""
    listed = {}
    for line in __doc__.splitlines():
        f = line.split()
        if len(f) >= 8 and f[0] in ("seam_weighted", "diag_needle"):
            listed[tuple(f[:4])] = (float(f[4]), float(f[5]))
    rows = summary_table()
    assert len(listed) == len(rows)
    for *key, mut, emu in rows:
        assert listed[tuple(key)] == pytest.approx(
            (mut, emu), rel=1e-2, abs=0.006), key
        if key[2] in NOT_SEPARABLE.get((key[0], key[1], key[3]), ()):
            assert mut < CAUGHT, "separable after all: unlist it"


def summary_table(randn=False):
    """Rows (family, mutant, stage, dtype, min-over-shapes of the mutant's
    worst ratio, max-over-shapes of the emulation's worst ratio): the
    module docstring's table."""
    rows = []
    for family in ("seam_weighted", "diag_needle"):
        cases = [c for c in CASES if c.family == family]
        for dtype in DTYPES:
            for mut in mo.MUTANTS:
                for stage in _stages(mut):
                    e = _EMU_OF.get(stage, "emu")
                    emu = max(max(evaluate(c, dtype, randn)[e].values())
                              for c in cases if e in evaluate(c, dtype, randn))
                    hit = [max(evaluate(c, dtype, randn)[mut.name, stage]
                               .values())
                           for c in cases
                           if (mut.name, stage) in evaluate(c, dtype, randn)]
                    if hit:
                        rows.append((family, mut.name, stage, _dt(dtype),
                                     min(hit), emu))
    return rows
