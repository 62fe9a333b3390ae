"""CPU checks of the boundary input helpers themselves: the families put
the mass where they say, poisoned_parent's views have the geometry the
GPU tests rely on, the carry-in references of boundary_refs.py (plain,
shifted, and the backward under the merged lse) are the eager softmax and
its gradient over [round-1 keys under its mask | round-2 keys under
theirs], and a dominated round keeps its distance from the carried max."""

import math

import pytest
import torch

from . import boundary_inputs as bi
from . import mutant_oracle as mo
from .gqa_cpu_provider import expand_kv
from .boundary_refs import (carry_ref as _carry_ref, inputs as _inputs,
                            merged_bwd_ref as _merged_bwd_ref,
                            round2_kv as _round2_kv,
                            shifted_ref as _shifted_ref)

S328 = [c for c in bi.CASES if c.sq == 328 and c.d == 128 and c.n == 4]


def _probs(q, k, scale, causal):
    n = q.shape[2]
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), expand_kv(k, n).float())
    s = s * scale
    if causal:
        s = s.masked_fill(~torch.ones(s.shape[-2:], dtype=torch.bool).tril(),
                          float("-inf"))
    return torch.softmax(s, -1)


def test_seam_keys_carry_the_mass():
    case = next(c for c in S328 if c.family == "seam_weighted"
                and not c.causal)
    q, k, _, do = _inputs(case, torch.float32)
    p = _probs(q, k, 1 / math.sqrt(case.d), False)
    share = p[..., bi.seam_keys(case.sk)]
    # nine seam keys at about the weight of all ordinary keys each
    assert share.sum(-1).median() > 0.8
    assert share.median() > 0.05
    rows = bi.seam_rows(case.sq)
    rest = [i for i in range(case.sq) if i not in rows]
    assert do[:, rows].std() / do[:, rest].std() == pytest.approx(
        bi.DO_GAIN, rel=0.1)


def test_diag_needle_scores():
    case = next(c for c in S328 if c.family == "diag_needle")
    q, k, _, _ = _inputs(case, torch.float32)
    s = torch.einsum("bqhd,bkhd->bhqk", q, expand_kv(k, case.n))
    s = s / math.sqrt(case.d)
    a = math.log(case.sq)
    g = case.n // case.nk
    first = s[:, ::g]  # the heads the keys were built from
    diag = first.diagonal(dim1=-2, dim2=-1)[..., 1:]
    sup = first.diagonal(1, dim1=-2, dim2=-1)
    # eps and cross terms: sd ~ sqrt(1 + (a^2 + c^2) / d) ~ 1.6
    assert (diag.mean() - a).abs() < 0.3 and (sup.mean() - 2 * a).abs() < 0.3
    p = _probs(q, k, 1 / math.sqrt(case.d), True)
    assert p[:, ::g].diagonal(dim1=-2, dim2=-1)[..., 200:].median() > 0.05


@pytest.mark.parametrize("lag", [0, 1, 3])
def test_diag_needle_lag_scores(lag):
    """The hot allowed key sits lag behind the row, the hotter forbidden
    one max(lag, 1) ahead; lag = 0 is the unlagged family bit for bit."""
    b, s, n, nk, d = 1, 328, 4, 2, 128
    q, k, v, do = bi.diag_needle(b, s, n, nk, d, torch.float32, 5, lag=lag)
    if lag == 0:
        for t, t0 in zip((q, k, v, do),
                         bi.diag_needle(b, s, n, nk, d, torch.float32, 5)):
            assert torch.equal(t, t0)
    sc = torch.einsum("bqhd,bkhd->bhqk", q, expand_kv(k, n)) / math.sqrt(d)
    first = sc[:, ::n // nk]
    a, ahead = math.log(s), max(lag, 1)
    hot = first.diagonal(-lag, dim1=-2, dim2=-1)
    forbidden = first.diagonal(ahead, dim1=-2, dim2=-1)
    assert hot.shape[-1] == s - lag and forbidden.shape[-1] == s - ahead
    assert (hot.mean() - a).abs() < 0.3
    assert (forbidden.mean() - 2 * a).abs() < 0.3


@pytest.mark.parametrize("which", ["below", "above"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16],
                         ids=bi.dtype_name)
@pytest.mark.parametrize("case", bi.DOMINATED_CASES, ids=bi.case_id)
def test_dominated_round_gap(case, dtype, which):
    """Every score of the dominated causal round is at least 30 from the
    row's carried max, on the side asked for."""
    q, k, _, _ = _inputs(case, dtype)
    k2, _ = bi.dominated_kv(case, dtype, which)
    tril = torch.ones(case.sq, case.sk, dtype=torch.bool).tril()
    score = lambda kk: torch.einsum(
        "bqhd,bkhd->bhqk", q.float(), expand_kv(kk, case.n).float()
    ) / math.sqrt(case.d)
    m1 = score(k).masked_fill(~tril, float("-inf")).amax(-1)
    s2 = score(k2)
    if which == "below":
        gap = m1 - s2.masked_fill(~tril, float("-inf")).amax(-1)
    else:
        gap = s2.masked_fill(~tril, float("inf")).amin(-1) - m1
    assert gap.min() >= bi.DOMINATED_MIN_GAP and gap.max() <= 130.0


def test_poisoned_parent_geometry():
    case = next(c for c in S328 if c.family == "seam_weighted" and c.causal)
    dtype = torch.float16
    ins = _inputs(case, dtype)
    P = bi.poisoned_parent(*ins)
    for name, t in zip(("q", "k", "v", "do"), ins):
        view, parent = P.views[name], P.parents[name]
        assert torch.equal(view, t) and not view.is_contiguous()
        # the binding layer's contract: 16-byte rows, head_dim contiguous
        assert view.stride(3) == 1
        assert view.stride(1) % 8 == 0 and view.stride(2) % 8 == 0
        assert view.storage_offset() % 8 == 0 and view.storage_offset() > 0
        assert view.stride(0) == 2 * parent.stride(0)
        inside = torch.zeros_like(parent, dtype=torch.bool)
        bi.view_of(inside, view, parent).fill_(True)
        assert inside.sum() == t.numel()
        outside = parent[~inside].float()
        want = bi.K_POISON if name in ("q", "k") else bi.V_POISON
        assert bool((outside.abs() == want).all())
        assert torch.isfinite(outside).all()
    for name, view in P.out_views.items():
        assert bool((P.out_parents[name] == bi.SENTINEL).all())
        assert view.stride(-1) == 1
    assert P.out_views["m"].stride() == P.out_views["l"].stride()
    assert P.out_views["dk"].shape == ins[1].shape
    assert P.out_views["m"].shape == (case.b, case.n, case.sq)


@pytest.mark.parametrize(
    "case", [c for c in bi.CASES if c.causal and c.n == 4 and c.d == 64
             and c.sq in (33, 328)],
    ids=bi.case_id)
def test_shifted_references_are_masked_eager(case):
    """shifted_ref and merged_bwd_ref against the eager softmax and its
    gradient over [k under tril | k2[:-1] under the shifted tril]: the two
    tiles differentiated under the merged lse and delta add up to the
    gradient of the whole row."""
    dtype = torch.float32
    q, k, v, do = _inputs(case, dtype)
    k2, v2 = _round2_kv(case, dtype)
    sq, sk = case.sq, case.sk
    ctx = mo.Ctx(case.b, sq, 2 * sk - 1, case.n, case.nk, False)
    spec = mo.base_spec(ctx)
    spec.allow[:, :sk] = torch.ones(sq, sk, dtype=torch.bool).tril()
    spec.allow[0, sk:] = False
    spec.allow[1:, sk:] = torch.ones(sq - 1, sk - 1, dtype=torch.bool).tril()
    kk, vv = torch.cat([k, k2[:, :-1]], 1), torch.cat([v, v2[:, :-1]], 1)
    scale = 1 / math.sqrt(case.d)
    o, lse = mo.forward(q, kk, vv, scale, spec)
    o_ref, lse_ref = _shifted_ref(case, dtype)
    torch.testing.assert_close(o_ref, o, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(lse_ref, lse, rtol=1e-5, atol=1e-5)
    dq, dk, dv = mo.backward(do, q, kk, vv, o, lse, scale, spec)
    dq_r, dk_r, dv_r, dk2_r, dv2_r = _merged_bwd_ref(case, dtype)
    tol = dict(rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(dq_r, dq, **tol)
    torch.testing.assert_close(dk_r, dk[:, :sk], **tol)
    torch.testing.assert_close(dv_r, dv[:, :sk], **tol)
    torch.testing.assert_close(dk2_r[:, :-1], dk[:, sk:], **tol)
    torch.testing.assert_close(dv2_r[:, :-1], dv[:, sk:], **tol)
    assert not dk2_r[:, -1].any() and not dv2_r[:, -1].any()


@pytest.mark.parametrize("case", S328, ids=lambda c: f"{c.family}-{c.causal}")
def test_carry_reference_is_masked_eager(case):
    """fp32 inputs, so the two fp32 restatements agree to roundoff."""
    dtype = torch.float32
    q, k, v, _ = _inputs(case, dtype)
    k2, v2 = _round2_kv(case, dtype)
    ctx = mo.Ctx(case.b, case.sq, 2 * case.sk, case.n, case.nk, False)
    spec = mo.base_spec(ctx)
    if case.causal:
        spec.allow[:, :case.sk] = torch.ones(
            case.sq, case.sk, dtype=torch.bool).tril()
    o, lse = mo.forward(q, torch.cat([k, k2], 1), torch.cat([v, v2], 1),
                        1 / math.sqrt(case.d), spec)
    o_ref, lse_ref = _carry_ref(case, dtype)
    torch.testing.assert_close(o_ref, o, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(lse_ref, lse, rtol=1e-5, atol=1e-5)
