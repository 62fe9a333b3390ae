"""The HIP kernels in the forms the ring's rounds give them, on ONE GPU.

``ring_rounds.replay_ring`` drives ``HipTileProvider`` through W virtual
ranks with exactly the calls the ring driver makes at W > 1: causal and
unmasked carry-in ``fwd_accum`` on the ``tile_window`` views (the zigzag
``row_offset = half`` windows, the striped one-token-shifted ones, whose
m/l rows start 4 bytes into their parent rows), ``fwd_finalize``, and
``bwd_accum`` under the whole-sequence lse and delta into accumulators
shared by W rounds.  The result is held to the fp32 full-sequence oracle
(``gqa_full_reference``; ``mutant_oracle.forward`` for lse) by the gates
of tests/test_gpu_parity.py (``boundary_refs.gates``).

The inputs are ``ring_rounds.CASES``: ``diag_needle`` with a lag, generated
on the full sequence, so that each row's hot allowed key and hotter
forbidden key sit on another rank, at that round's tile boundary; per-rank
length 330 makes every window ragged (see ``ring_rounds.S_LOCAL``).
tests/test_ring_rounds_cpu.py proves on the CPU that on these cases the
gates reject a one-pair or one-row error in any of those forms and pass
low-precision rounding.

Each causal case also runs the stateless form (``ring_sim.simulate_ring``:
``fwd`` / ``bwd`` per tile and a python merge) against the same reference,
so a failure says whether the accumulate form or the tile is wrong.

Every check prints ``GATE ring[-stateless] <case> <dtype> <output>
<ratio>`` (shown under ``-s``); profiles/gate_sensitivity/README.md records
them.
"""

import functools

import pytest
import torch

from . import mutant_oracle as mo
from . import ring_rounds as rr
from .boundary_inputs import dtype_name as _dt
from .boundary_refs import gates
from .gqa_cpu_provider import gqa_full_reference
from .ring_sim import simulate_ring

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
# both values of `deterministic` on the W = 4 cases; (case, dtype) varies
# slowest, so the shared reference is computed once and then dropped
PARAMS = [(c, t, det) for c in rr.CASES for t in DTYPES
          for det in ((False, True) if c.W == 4 else (False,))]
RING = pytest.mark.parametrize(
    "case,dtype,det", PARAMS,
    ids=[f"{rr.case_id(c)}-{_dt(t)}-{'det' if det else 'atomic-ok'}"
         for c, t, det in PARAMS])


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
    """Print every output's worst gate ratio for every form, then assert
    the gates, in the order given."""
    gt = gates(dtype, case.n // case.nk)
    refs = _reference(case, dtype)
    triples = [(test, name, out.float().cpu())
               for test, outs in forms for name, out in outs.items()]
    for test, name, out in triples:
        print(f"GATE {test} {rr.case_id(case)} {_dt(dtype)} {name} "
              f"{mo.gate_ratio(out, refs[name], **gt[name]):.3f}")
    for test, name, out in triples:
        torch.testing.assert_close(
            out, refs[name], msg=lambda m: f"{test} {name}: {m}", **gt[name])


@RING
def test_ring_rounds(case, dtype, det):
    from burst_attn_amd.tile import HipTileProvider

    P = HipTileProvider()
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
        forms.append(("ring-stateless",
                      {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}))
    _check(case, dtype, forms + [("ring", accum)])
