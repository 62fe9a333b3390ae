"""The band reference and its inputs, on the CPU (tests/window_refs.py).

Sensitivity: for the three needle cases, the reference under each of the four
bands that are one off at one edge misses the gate of EVERY output of the
reference under the true band: a kernel whose band test is off by one at
either edge cannot pass tests/test_gpu_window.py.  Rounding: what a correct
low-precision kernel does still passes.  Dead rows: rows that see nothing
and keys seen by nobody are exact zeros and -inf.
"""

import math

import pytest
import torch

from . import segment_refs as sr
from . import window_refs as wr
from .boundary_refs import gates
from .gqa_cpu_provider import expand_kv

DTYPES = [torch.float16, torch.bfloat16]
OUTS = ("o", "lse", "dq", "dk", "dv")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_band_one_off_misses_every_gate(name, dtype):
    case = wr.CASES[name]
    c = wr.table_case(name, dtype)
    gt = gates(dtype, case.n // case.nk)
    lo, hi = case.lo, case.hi
    for mlo, mhi in ((lo - 1, hi), (lo + 1, hi), (lo, hi - 1), (lo, hi + 1)):
        wrong = wr.band_ref(c, mlo, mhi)
        worst = {nm: sr.exceeds(wrong[nm], c[nm], gt[nm]) for nm in OUTS}
        print(f"MUTANT {name} {dtype} ({mlo},{mhi}) "
              + " ".join(f"{nm}={x:.1f}" for nm, x in worst.items()))
        assert min(worst.values()) > 1.0, ((mlo, mhi), worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_low_precision_rounding_passes_the_gates(name, dtype):
    """P rounded to the input dtype before the PV product, and the reference
    o itself rounded to it."""
    case = wr.CASES[name]
    c = wr.table_case(name, dtype)
    gt = gates(dtype, case.n // case.nk)
    q = c["q"].float().transpose(1, 2)
    k = expand_kv(c["k"], case.n).float().transpose(1, 2)
    v = expand_kv(c["v"], case.n).float().transpose(1, 2)
    m = c["mask"][:, None]
    s = (q @ k.transpose(-1, -2) * c["scale"]).masked_fill(~m, float("-inf"))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = (p.to(dtype).float() @ v) / p.sum(-1, keepdim=True)
    assert sr.exceeds(o.transpose(1, 2), c["o"], gt["o"]) <= 1.0
    # o is the one output that exists in the input dtype (the ring's out)
    assert sr.exceeds(c["o"].to(dtype).float(), c["o"], gt["o"]) <= 1.0


def test_dead_rows_and_unseen_keys_are_exact():
    d = wr.table_case("d", torch.float16)
    for nm in ("dk", "dv"):
        assert (d[nm][:, 96:] == 0).all(), nm
        assert d[nm][:, :96].abs().sum() > 0
    assert d["lse"].isfinite().all()
    e = wr.table_case("e", torch.float16)
    assert (e["o"][:, :200] == 0).all()
    assert (e["lse"][:, :, :200] == -math.inf).all()
    assert (e["dq"][:, :200] == 0).all()
    assert e["lse"][:, :, 200:].isfinite().all()
    # keys 128.. are seen by nobody (row 327 sees keys up to 127)
    assert (e["dk"][:, 128:] == 0).all() and (e["dv"][:, 128:] == 0).all()
    for c in (d, e):
        for nm in ("o", "dq", "dk", "dv"):
            assert c[nm].isfinite().all(), nm


@pytest.mark.parametrize("causal", [False, True])
def test_global_window_mask(causal):
    S = 9
    for left, right in ((0, 0), (2, 1), (-1, 0), (0, -1), (-1, -1), (3, 20)):
        m = wr.global_window_mask(S, left, right, causal)
        for i in range(S):
            for j in range(S):
                r = 0 if causal else right
                want = (left < 0 or j >= i - left) and (r < 0 or j <= i + r)
                assert bool(m[i, j]) == want, (left, right, i, j)


def test_band_mask_is_the_global_mask_of_a_square():
    assert torch.equal(wr.band_mask(1, 7, 7, -2, 3)[0],
                       wr.global_window_mask(7, 3, 2, False))


# ---- the one-GPU ring replay's helper, on the oracle provider ----------------

@pytest.mark.parametrize("window,causal", [((100, 0), True),
                                           ((60, 60), False)])
def test_window_replay_helper_on_cpu(window, causal):
    """tests/window_ring_rounds.replay_window_ring composes the product's
    window_tiles sub-tiles to the full-sequence reference, in all three
    layouts."""
    from . import window_ring_rounds as wrr
    from .window_cpu_provider import WindowOracleTileProvider

    c = wrr.ring_case(3, window, causal, 64, torch.float32)
    for layout in ("zigzag", "contiguous", "striped"):
        got = wrr.replay_window_ring(WindowOracleTileProvider(), c["q"],
                                     c["k"], c["v"], c["do"], 3, c["scale"],
                                     causal, layout, window)
        for name, out in zip(OUTS, got):
            torch.testing.assert_close(
                out, c[name], rtol=1e-4, atol=1e-4,
                msg=lambda m, name=name: f"{layout} {name}: {m}")
