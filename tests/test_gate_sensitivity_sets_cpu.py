"""CPU proof for tests/test_gpu_boundary_sets.py: on
``boundary_inputs.SET_CASES`` (head_dim 256, and q/k 192 with v 128) the
parity gates separate a one-predicate error from low-precision rounding.

The criteria, CAUGHT / CLEAN and the two documented exceptions are those
of tests/test_gate_sensitivity_cpu.py, whose ``evaluate`` does the scoring:
every applicable mutant of ``mutant_oracle.MUTANTS`` and of
``mutant_oracle.BLOCK128_MUTANTS`` (the workgroup-seam errors at row 128,
where these kernel sets have their block edge) scores >= CAUGHT on at least
one output its stage asserts, in every case, and the rounding emulation of
the unmutated math scores <= CLEAN on every output.  No exception is added:
the ``full_subtile_early`` entries of NOT_SEPARABLE hold here for the reason
given there (on seam_weighted a diagonal subtile taken as full leaks
ordinary keys only), and likewise for its row-128 twin on the same family,
which therefore shares its entries.
"""

import pytest
import torch

from . import mutant_oracle as mo
from .boundary_inputs import SET_CASES, case_id as _id, dtype_name as _dt
from .test_gate_sensitivity_cpu import (CAUGHT, CLEAN, EMU, NOT_SEPARABLE,
                                        evaluate)

DTYPES = [torch.float16, torch.bfloat16]
MUTANTS = tuple(mo.MUTANTS + mo.BLOCK128_MUTANTS)
# the row-128 twin of a listed mutant is the same error at another seam
_TWIN = {"block128_subtile_early": "full_subtile_early"}


def _evaluate(case, dtype):
    return evaluate(case, dtype, block128=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("case", SET_CASES, ids=_id)
def test_mutants_rejected(case, dtype):
    missed = []
    for key, ratios in _evaluate(case, dtype).items():
        if key in EMU:
            continue
        name = _TWIN.get(key[0], key[0])
        if key[1] in NOT_SEPARABLE.get((case.family, name, _dt(dtype)), ()):
            continue
        if max(ratios.values()) < CAUGHT:
            missed.append((key, ratios))
    assert not missed, missed


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("case", SET_CASES, ids=_id)
def test_rounding_emulation_passes(case, dtype):
    res = _evaluate(case, dtype)
    over = {(e, k): r for e in EMU if e in res for k, r in res[e].items()
            if r > CLEAN}
    assert not over, over


def test_every_mutant_applies_somewhere():
    """At both width pairs every mutant meets a shape with its seam in it."""
    for d in (256, 192):
        seen = set()
        for case in SET_CASES:
            if case.d == d:
                seen |= {k[0] for k in _evaluate(case, torch.bfloat16)
                         if k not in EMU}
        assert seen == {m.name for m in MUTANTS}, d
