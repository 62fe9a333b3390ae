"""The tile-level ring forms of tests/test_gpu_boundary.py on the head_dim
256, 192 / 128 and fp8 kernel sets.

Those sets are separate code with 128-row workgroups of their own, and
their own tests run one non-causal two-round carry-in.  Here they get the
forms the ring's later rounds hand a kernel: the stateless call, the
carry-in call (masked round first, and causal with carried state, the
striped order), the call on views shifted by one token (m/l rows 4 bytes
into their parents), the rescale of carried state by a round that
dominates it or is dominated by it, and, for the 16-bit sets, the backward
under an lse and delta that belong to more keys than the tile's, both
rounds adding into one dq through shifted dq/dk/dv views.

16-bit sets: ``boundary_inputs.SET_CASES`` (the families of
``boundary_inputs.CASES`` with the 127 / 128 block-seam keys and rows added,
at shapes below one 128-row block, one row past it, and 328), the
references of tests/boundary_refs.py and the unchanged gates of
tests/test_gpu_parity.py.  tests/test_gate_sensitivity_sets_cpu.py proves
on the CPU that on these cases the gates reject a one-predicate error.

fp8 (per-tensor floats and block-scaled tensors), forward forms only, on
an exact-P family: softmax_scale = ln 2, q rows one-hot over channels
0..126 and 1 in the reserved channel 127, integer k entries, so every
exp2-domain score is an integer, every P a power of two, and the fp64
reference on the dequantised inputs is the kernel's own arithmetic: the
16-bit gates TOL[fp16] and LSE_TOL apply unchanged.  Causal cases are a
needle (0 on the row's own key, +3 on the key after it, -8 elsewhere);
unmasked ones have k in {0..-3} with +3 on the seam keys.  The reserved
channel is 0 in k, except in a dominated second round, where +-48 puts
every score 42 or more below / above the carried max and +160 makes the
carried side vanish (exp2(-149) is fp32's last subnormal).  The
block-scaled calls re-express the same values in power-of-two scales per
row, tile and channel, so both share one reference.

Each check prints ``GATE sets-<test> <case> <dtype> <output> <ratio>``.
"""

import functools
import math

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
from .test_gpu_parity import LSE_TOL, TOL

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
_set_id = lambda c: f"{bi.kernel_set(c)}-{_id(c)}"
CASES = pytest.mark.parametrize("case", bi.SET_CASES, ids=_set_id)
CAUSAL_CASES = pytest.mark.parametrize(
    "case", [c for c in bi.SET_CASES if c.causal], ids=_set_id)
SHIFT_CASES = pytest.mark.parametrize(
    "case", [c for c in bi.SET_CASES if c.causal and c.sq >= 2], ids=_set_id)
BY_DTYPE = pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
BY_DET = pytest.mark.parametrize("det", [False, True],
                                 ids=["atomic-ok", "det"])


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
        print(f"GATE sets-{test} {_set_id(case)} {_dt(dtype)} {name} "
              f"{gate_ratio(out, ref, **gt[name]):.3f}")
    for name, out, ref in pairs:
        assert out.shape == ref.shape, (name, out.shape, ref.shape)
        torch.testing.assert_close(out, ref, msg=lambda m: f"{name}: {m}",
                                   **gt[name])


def _state(b, sq, n, d):
    acc = torch.empty(b, sq, n, d, dtype=torch.float32, device="cuda")
    m = torch.empty(b, n, sq, dtype=torch.float32, device="cuda")
    return acc, m, torch.empty_like(m)


def _state_of(case):
    return _state(case.b, case.sq, case.n, bi.v_dim(case))


def _named(o_lse):
    return dict(zip(("o", "lse"), o_lse))


def _named_grads(g):
    return dict(zip(("dq", "dk", "dv"), g))


# ---- 16-bit sets, forward

@BY_DTYPE
@CASES
def test_fwd_stateless(case, dtype):
    q, k, v, _ = _gpu(*_inputs(case, dtype))
    o, lse = _ext().attn_fwd(q, k, v, _scale(case), case.causal)
    _check("fwd", case, dtype, {"o": o, "lse": lse},
           _named(_fwd_ref(case, dtype)))


@BY_DTYPE
@CASES
def test_fwd_carry_in(case, dtype):
    """A fresh accumulator under the case's mask, then round 2 unmasked
    merged in-kernel, then finalize."""
    ext = _ext()
    q, k, v, _ = _gpu(*_inputs(case, dtype))
    k2, v2 = _gpu(*_round2_kv(case, dtype))
    acc, m, l = _state_of(case)
    ext.attn_fwd_accum(q, k, v, _scale(case), case.causal, acc, m, l, False)
    ext.attn_fwd_accum(q, k2, v2, _scale(case), False, acc, m, l, True)
    o, lse = ext.attn_fwd_finalize(acc, m, l, dtype)
    _check("carry", case, dtype, {"o": o, "lse": lse},
           _named(_carry_ref(case, dtype)))


@BY_DTYPE
@CAUSAL_CASES
def test_fwd_carry_in_causal(case, dtype):
    """The striped order: a fresh unmasked round on round2_kv, then the
    case's keys merged in under the causal mask, with carried state."""
    ext = _ext()
    q, k, v, _ = _gpu(*_inputs(case, dtype))
    k2, v2 = _gpu(*_round2_kv(case, dtype))
    acc, m, l = _state_of(case)
    ext.attn_fwd_accum(q, k2, v2, _scale(case), False, acc, m, l, False)
    ext.attn_fwd_accum(q, k, v, _scale(case), True, acc, m, l, True)
    o, lse = ext.attn_fwd_finalize(acc, m, l, dtype)
    _check("carry-causal", case, dtype, {"o": o, "lse": lse},
           _named(_carry_ref(case, dtype)))


def _shifted_state(case, dtype):
    """(acc, m, l) after a fresh causal round on (k, v) and the shifted
    causal carry-in round on round2_kv."""
    ext = _ext()
    q, k, v, _ = _gpu(*_inputs(case, dtype))
    k2, v2 = _gpu(*_round2_kv(case, dtype))
    acc, m, l = _state_of(case)
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
@pytest.mark.parametrize("case", bi.SET_DOMINATED_CASES, ids=_set_id)
def test_fwd_carry_in_dominated(case, dtype, which):
    """A causal carry-in round whose every score is 30 or more below the
    carried max (the result is round 1, to within the gate) or above it
    (the carried acc and l must vanish without leaving inf or nan)."""
    ext = _ext()
    q, k, v, _ = _gpu(*_inputs(case, dtype))
    k2, v2 = _gpu(*_dominated_kv(case, dtype, which))
    acc, m, l = _state_of(case)
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


# ---- 16-bit sets, backward

@BY_DET
@BY_DTYPE
@CASES
def test_bwd_default_plan(case, dtype, det):
    ext = _ext()
    q, k, v, do = _gpu(*_inputs(case, dtype))
    o, lse = ext.attn_fwd(q, k, v, _scale(case), case.causal)
    delta = ext.attn_bwd_preprocess(o.to(dtype), do)
    dq, dk, dv = ext.attn_bwd(do, q, k, v, delta, lse, _scale(case),
                              case.causal, det)
    _check("bwd", case, dtype, {"dq": dq, "dk": dk, "dv": dv},
           _named_grads(_bwd_ref(case, dtype)))


@BY_DET
@BY_DTYPE
@SHIFT_CASES
def test_bwd_accum_under_merged_lse(case, dtype, det):
    """lse and delta belong to the merged two-round forward of
    test_fwd_carry_in_shifted; both rounds' tiles accumulate into one dq,
    the second through the shifted views delta[:, :, 1:], lse[:, :, 1:],
    dq[:, 1:] and dk2/dv2[:, :-1]."""
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


# ---- fp8: forward forms on the exact-P family

FP8 = torch.float8_e4m3fn
D, RESERVED = 128, 127
LN2 = math.log(2.0)
F16 = TOL[torch.float16]
# (sq, sk, n, nk, causal): the shapes of boundary_inputs.SET_CASES
FP8_SHAPES = sorted({(c.sq, c.sk, c.n, c.nk, c.causal) for c in bi.SET_CASES})
B = 2
DOMINATED = {"below": -48.0, "above": 48.0, "vanish": 160.0}
MODES = pytest.mark.parametrize("mode", ["fp8", "fp8_scaled"])


def _shape_id(shape):
    sq, sk, n, nk, causal = shape
    return f"{sq}x{sk}-n{n}k{nk}-{'causal' if causal else 'full'}"


def _shapes(keep=lambda s: True):
    return pytest.mark.parametrize(
        "shape", [s for s in FP8_SHAPES if keep(s)], ids=_shape_id)


@functools.lru_cache(maxsize=None)
def _fp8_tensors(shape, round2=False, reserved=0.0):
    """fp32 (q, k, v) of the exact-P family, every value an e4m3 value."""
    sq, sk, n, nk, causal = shape
    g = torch.Generator().manual_seed(880 + sq + 3 * sk + nk + 7 * round2)
    i, j = torch.arange(sq), torch.arange(sk)
    q = torch.zeros(B, sq, n, D)
    q[:, i, :, i % RESERVED] = 1.0
    q[..., RESERVED] = 1.0
    if causal and not round2:
        k = torch.full((B, sk, nk, D), -8.0)
        k[:, j, :, j % RESERVED] = 0.0
        k[:, j, :, (j - 1) % RESERVED] = 3.0
    else:
        k = -torch.randint(0, 4, (B, sk, nk, D), generator=g).float()
        k[:, bi.seam_keys(sk, bi.BLOCK_SEAMS)] = 3.0
    k[..., RESERVED] = reserved
    v = torch.randn(B, sk, nk, D, generator=g).to(FP8).float()
    # what stays a normal e4m3 number when re-expressed in units 4x larger
    v[v.abs() < 2.0 ** -4] = 0.0
    return q, k, v


def _quantise(q, k, v, mode):
    """(q8, k8, v8, descale) on the GPU whose dequantised values are q, k
    and v / 4: three floats, or power-of-two scale tensors per q row, k
    tile and v channel with the e4m3 values scaled to match, exactly."""
    if mode == "fp8":
        return (*_gpu(*(t.to(FP8) for t in (q, k, v))), (1.0, 1.0, 0.25))
    sq, sk, n, nk = q.shape[1], k.shape[1], q.shape[2], k.shape[2]
    eq = (torch.arange(sq)[None, None] + torch.arange(n)[None, :, None]
          + torch.arange(B)[:, None, None]) % 3            # [B, N, Sq]
    ek = (torch.arange(-(-sk // 64))[None, None]
          + torch.arange(nk)[None, :, None]
          + torch.arange(B)[:, None, None]) % 2            # [B, Nk, tiles]
    ev = (torch.arange(D)[None, None] + torch.arange(nk)[None, :, None]) % 4
    ev = ev.expand(B, nk, D)                               # [B, Nk, D]
    q8 = q * 2.0 ** eq.transpose(1, 2)[..., None]
    k8 = k * 2.0 ** ek.repeat_interleave(64, 2)[:, :, :sk].transpose(
        1, 2)[..., None]
    v8 = v * 2.0 ** (ev[:, None] - 2.0)  # |v| <= 448 / 4 after the shift
    for t in (q8, k8, v8):
        assert torch.equal(t.to(FP8).float(), t), "not an e4m3 value"
    ds = tuple((2.0 ** -e.float()).contiguous().cuda() for e in (eq, ek, ev))
    return (*_gpu(*(t.to(FP8) for t in (q8, k8, v8))), ds)


def _fp8_ref(q, rounds):
    """fp64 (o, lse [B,N,S]) of one softmax over the rounds' keys, each
    round a (k, v, allow [Sq, Sk]) of fp32 values; v enters as v / 4."""
    g = q.shape[2] // rounds[0][0].shape[2]
    ke, ve = (torch.cat([r[i].double().repeat_interleave(g, dim=2)
                         for r in rounds], 1) for i in (0, 1))
    allow = torch.cat([r[2] for r in rounds], 1)
    s = torch.einsum("bqnd,bknd->bnqk", q.double(), ke) * LN2
    s = s.masked_fill(~allow, -math.inf)
    o = torch.einsum("bnqk,bknd->bqnd", torch.softmax(s, -1), ve * 0.25)
    return o.float(), torch.logsumexp(s, -1).float()


def _fp8_check(test, shape, mode, o, lse, ref):
    outs = {"o": (o, ref[0], F16), "lse": (lse, ref[1], LSE_TOL)}
    for name, (out, r, gate) in outs.items():
        print(f"GATE sets-{test} {mode}-{_shape_id(shape)} fp8 {name} "
              f"{gate_ratio(out.float().cpu(), r, **gate):.3f}")
    for name, (out, r, gate) in outs.items():
        torch.testing.assert_close(out.float().cpu(), r,
                                   msg=lambda m: f"{name}: {m}", **gate)


def _mask(sq, sk, causal):
    m = torch.ones(sq, sk, dtype=torch.bool)
    return m.tril() if causal else m


def _shift_mask(sq, sk):
    """Rows 1.. against keys ..-1 under the causal mask; the last key is
    not part of the call."""
    m = torch.zeros(sq, sk, dtype=torch.bool)
    m[1:, :sk - 1] = torch.ones(sq - 1, sk - 1, dtype=torch.bool).tril()
    return m


@MODES
@_shapes()
def test_fp8_stateless(shape, mode):
    from burst_attn_amd.tile import HipTileProvider

    sq, sk, _, _, causal = shape
    q, k, v = _fp8_tensors(shape)
    q8, k8, v8, ds = _quantise(q, k, v, mode)
    o, lse = HipTileProvider().fwd(q8, k8, v8, LN2, causal, descale=ds)
    _fp8_check("fwd", shape, mode, o, lse,
               _fp8_ref(q, [(k, v, _mask(sq, sk, causal))]))


def _two_rounds(shape, mode, first, second, reserved=0.0, shifted=False):
    """(acc, m, l, (o, lse), ref) of two accumulate calls: `first` and
    `second` are (round2 keys?, causal) of each call."""
    ext = _ext()
    sq, sk, n, _, _ = shape
    q = _fp8_tensors(shape)[0]
    acc, m, l = _state(B, sq, n, D)
    rounds = []
    for idx, (round2, causal) in enumerate((first, second)):
        _, k, v = _fp8_tensors(shape, round2, reserved if idx else 0.0)
        q8, k8, v8, ds = _quantise(q, k, v, mode)
        if idx and shifted:
            if mode == "fp8_scaled":
                ds = (ds[0][:, :, 1:], ds[1], ds[2])
            ext.attn_fwd_accum(q8[:, 1:], k8[:, :-1], v8[:, :-1], LN2, True,
                               acc[:, 1:], m[:, :, 1:], l[:, :, 1:], True,
                               descale=ds)
            rounds.append((k, v, _shift_mask(sq, sk)))
        else:
            ext.attn_fwd_accum(q8, k8, v8, LN2, causal, acc, m, l, bool(idx),
                               descale=ds)
            rounds.append((k, v, _mask(sq, sk, causal)))
    return acc, m, l, ext.attn_fwd_finalize(acc, m, l, torch.float16), \
        _fp8_ref(q, rounds)


@MODES
@_shapes()
def test_fp8_carry_in(shape, mode):
    *_, (o, lse), ref = _two_rounds(shape, mode, (False, shape[4]),
                                    (True, False))
    _fp8_check("carry", shape, mode, o, lse, ref)


@MODES
@_shapes(lambda s: s[4])
def test_fp8_carry_in_causal(shape, mode):
    *_, (o, lse), ref = _two_rounds(shape, mode, (True, False),
                                    (False, True))
    _fp8_check("carry-causal", shape, mode, o, lse, ref)


@MODES
@_shapes(lambda s: s[4] and s[0] >= 2)
def test_fp8_carry_in_shifted(shape, mode):
    *_, (o, lse), ref = _two_rounds(shape, mode, (False, True), (True, True),
                                    shifted=True)
    _fp8_check("carry-shifted", shape, mode, o, lse, ref)


@pytest.mark.parametrize("which", list(DOMINATED))
@MODES
@_shapes(lambda s: s == (328, 328, 4, 2, True))
def test_fp8_carry_in_dominated(shape, mode, which):
    acc, m, l, (o, lse), ref = _two_rounds(
        shape, mode, (False, True), (True, True), reserved=DOMINATED[which])
    for name, t in (("acc", acc), ("m", m), ("l", l), ("o", o), ("lse", lse)):
        assert bool(torch.isfinite(t).all()), name
    _fp8_check(f"carry-dominated-{which}", shape, mode, o, lse, ref)
    q, k, v = _fp8_tensors(shape)
    alone = _fp8_ref(q, [(k, v, _mask(shape[0], shape[1], True))])
    if which == "below":
        _fp8_check("carry-dominated-below-vs-round1", shape, mode, o, lse,
                   alone)
    if which == "vanish":  # nothing of round 1 is left
        _, k2, v2 = _fp8_tensors(shape, True, DOMINATED[which])
        only2 = _fp8_ref(q, [(k2, v2, _mask(shape[0], shape[1], True))])
        _fp8_check("carry-dominated-vanish-vs-round2", shape, mode, o, lse,
                   only2)


def test_fp8_scaled_carry_in_on_tile_offset_views():
    """A causal carry-in call as the zigzag ring's later half makes it: k
    and v are views that start 64 rows (one tile) into their tensors, dk
    the tiles from 1 on (interface._dk_tiles), and dq a window of a longer
    row, so its head stride is not its length."""
    from burst_attn_amd.interface import _dk_tiles

    ext = _ext()
    shape, mode = (328, 328, 4, 2, True), "fp8_scaled"
    sq, sk, n, nk, _ = shape
    q, k1, v1 = _fp8_tensors(shape, True)
    _, k, v = _fp8_tensors(shape)
    acc, m, l = _state(B, sq, n, D)
    q8, k8, v8, ds = _quantise(q, k1, v1, mode)
    ext.attn_fwd_accum(q8, k8, v8, LN2, False, acc, m, l, False, descale=ds)
    # round 2: the case's keys, embedded one tile into a longer tensor
    pad = lambda t: torch.cat([torch.full_like(t[:, :64], 3.0), t], 1)
    q8, k8, v8, (dq, dk, dv) = _quantise(q, pad(k), pad(v), mode)
    rows = slice(64, 64 + sk)
    dq_par = torch.full((B, n, sq + 9), float("nan"), device="cuda")
    dq_par[:, :, 5:5 + sq] = dq
    dq_view = dq_par[:, :, 5:5 + sq]
    assert not dq_view.is_contiguous() and not k8[:, rows].is_contiguous()
    ext.attn_fwd_accum(q8, k8[:, rows], v8[:, rows], LN2, True, acc, m, l,
                       True, descale=(dq_view, _dk_tiles(dk, rows, 64 + sk,
                                                         "test"), dv))
    o, lse = ext.attn_fwd_finalize(acc, m, l, torch.float16)
    ref = _fp8_ref(q, [(k1, v1, _mask(sq, sk, False)),
                       (k, v, _mask(sq, sk, True))])
    _fp8_check("carry-causal-tile-offset", shape, mode, o, lse, ref)
