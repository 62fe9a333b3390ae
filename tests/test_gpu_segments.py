"""The HIP kernels with segment ids (packed sequences), on one GPU.

Reference: the dense masked softmax of tests/segment_refs.py (pinned to the
oracle per document by tests/test_segments_cpu.py), on inputs whose
document boundaries carry hot keys with shifted V rows, so that one token
in the wrong document misses a gate (proved on the CPU there).  Gates:
``boundary_refs.gates``, those of tests/test_gpu_parity.py.
"""

import math

import pytest
import torch

from . import segment_refs as sr
from . import segment_ring_rounds as srr
from .boundary_inputs import dtype_name as _dt
from .boundary_refs import gates

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
HEADS = [(2, 2), (4, 2)]
SHAPE = pytest.mark.parametrize(
    "d,heads,dtype", [(d, h, t) for d in (64, 128) for h in HEADS
                      for t in DTYPES],
    ids=[f"d{d}-n{h[0]}k{h[1]}-{_dt(t)}" for d in (64, 128) for h in HEADS
         for t in DTYPES])


def _P():
    from burst_attn_amd.tile import HipTileProvider

    return HipTileProvider()


def _gpu(c, *names):
    return [c[n].cuda() for n in names]


def _run(P, q, k, v, do, scale, causal, seg):
    """Stateless forward, then the backward under its own lse and delta."""
    kw = {} if seg is None else {"seg": seg}
    o, lse = P.fwd(q, k, v, scale, causal, **kw)
    delta = P.bwd_preprocess(o.to(q.dtype), do)
    dq, dk, dv = P.bwd(do, q, k, v, delta, lse, scale, causal, False, **kw)
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def _assert_gates(got, ref, dtype, g, what):
    gt = gates(dtype, g)
    for name, out in got.items():
        out = out.float().cpu()
        print(f"GATE {what} {_dt(dtype)} {name} "
              f"{sr.exceeds(out, ref[name], gt[name]):.3f}")
    for name, out in got.items():
        torch.testing.assert_close(
            out.float().cpu(), ref[name], equal_nan=False,
            msg=lambda m, name=name: f"{what} {name}: {m}", **gt[name])


def _ref_with_kernel_delta(c, got, q_seg, kv_seg, causal, mask=None):
    """The reference gradients under the delta the backward was given
    (rowsum of o rounded to the input dtype times dO), as every tile test
    of this suite compares."""
    o16 = got["o"].to(c["q"].dtype).float().cpu()
    delta = (o16 * c["do"].float()).sum(-1).transpose(1, 2).contiguous()
    dq, dk, dv = sr.seg_bwd(c["do"], c["q"], c["k"], c["v"], c["lse"],
                            c["scale"], causal, q_seg, kv_seg, delta=delta,
                            mask=mask)
    return dict(o=c["o"], lse=c["lse"], dq=dq, dk=dk, dv=dv)


# ---- 1. tiles against the reference ----------------------------------------

@SHAPE
def test_causal_tile(d, heads, dtype):
    c = sr.causal_case(*heads, d, dtype)
    q, k, v, do, ids = _gpu(c, "q", "k", "v", "do", "q_seg")
    got = _run(_P(), q, k, v, do, c["scale"], True, (ids, ids))
    _assert_gates(got, _ref_with_kernel_delta(c, got, c["q_seg"], c["kv_seg"],
                                              True),
                  dtype, heads[0] // heads[1], "seg-causal")


@SHAPE
def test_rect_tile_and_never_visible_rows(d, heads, dtype):
    """Independent ids on the two sides; query id 9 has no key (o = 0,
    lse = -inf, dq exactly 0), kv documents 5 and 6 no query (dk = dv = 0);
    everything else finite."""
    c = sr.rect_case(*heads, d, dtype)
    q, k, v, do, qs, ks = _gpu(c, "q", "k", "v", "do", "q_seg", "kv_seg")
    got = _run(_P(), q, k, v, do, c["scale"], False, (qs, ks))
    dead = (c["q_seg"][0] == 9)
    unseen = (c["kv_seg"][0] == 5) | (c["kv_seg"][0] == 6)
    o, lse = got["o"].cpu(), got["lse"].cpu()
    assert (o[:, dead] == 0).all()
    assert (lse[:, :, dead] == -math.inf).all()
    assert (got["dq"].cpu()[:, dead] == 0).all()
    assert (got["dk"].cpu()[:, unseen] == 0).all()
    assert (got["dv"].cpu()[:, unseen] == 0).all()
    for name in ("o", "dq", "dk", "dv"):
        assert got[name].isfinite().all(), name
    assert lse[:, :, ~dead].isfinite().all()
    _assert_gates(got, _ref_with_kernel_delta(c, got, c["q_seg"], c["kv_seg"],
                                              False),
                  dtype, heads[0] // heads[1], "seg-rect")


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("d", [64, 128])
def test_striped_shift_views(d, dtype):
    """The striped ring's one-token shift: rows 1.. against keys ..-1 under
    the causal mask, ids sliced with the same windows (their base pointers
    are 4 bytes into the rows)."""
    c = sr.causal_case(4, 2, d, dtype)
    q, k, v, do, ids = _gpu(c, "q", "k", "v", "do", "q_seg")
    qv, kv, vv, dov = q[:, 1:], k[:, :-1], v[:, :-1], do[:, 1:]
    seg = (ids[:, 1:], ids[:, :-1])
    got = _run(_P(), qv, kv, vv, dov, c["scale"], True, seg)
    cs = {n: c[n][:, 1:] for n in ("q", "do")}
    cs.update({n: c[n][:, :-1] for n in ("k", "v")})
    qs, ks = c["q_seg"][:, 1:], c["kv_seg"][:, :-1]
    cs["scale"] = c["scale"]
    cs["o"], cs["lse"] = sr.seg_fwd(cs["q"], cs["k"], cs["v"], c["scale"],
                                    True, qs, ks)
    _assert_gates(got, _ref_with_kernel_delta(cs, got, qs, ks, True), dtype,
                  2, "seg-shift")


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("d", [64, 128])
def test_carry_in_row_offset_window(d, dtype):
    """Round 1: the causal tile.  Round 2: the zigzag window, rows half..
    against a second set of keys, unmasked but for the ids, carried into the
    state's row_offset views; its kv ids are a rotation (not sorted) without
    id 4, so rows 200..255 meet no key of round 2 and keep their state."""
    c = sr.causal_case(4, 2, d, dtype)
    P = _P()
    q, k, v, ids = _gpu(c, "q", "k", "v", "q_seg")
    half = sr.CAUSAL_S // 2
    g = torch.Generator().manual_seed(31 + d)
    k2 = torch.randn(c["k"].shape, generator=g).to(dtype)
    v2 = torch.randn(c["v"].shape, generator=g).to(dtype)
    ids2 = (c["kv_seg"] + 3) % 7          # ids 3, 4, 5, 6, 0, 1, 2: no order
    ids2[ids2 == 4] = 11
    state = P.fwd_accum(None, q, k, v, c["scale"], True, seg=(ids, ids))
    state = P.fwd_accum(state, q[:, half:], k2.cuda(), v2.cuda(), c["scale"],
                        False, row_offset=half,
                        seg=(ids[:, half:], ids2.cuda()))
    o, lse = P.fwd_finalize(state, dtype)
    m1 = sr.mask_of(c["q_seg"], c["kv_seg"], True)
    m2 = sr.mask_of(c["q_seg"], ids2, False)
    m2[:, :half] = False
    o_ref, lse_ref = sr.seg_fwd(c["q"], torch.cat([c["k"], k2], 1),
                                torch.cat([c["v"], v2], 1), c["scale"], False,
                                None, None, mask=torch.cat([m1, m2], 2))
    gt = gates(dtype, 2)
    torch.testing.assert_close(o.float().cpu(), o_ref, **gt["o"])
    torch.testing.assert_close(lse.cpu(), lse_ref, **gt["lse"])


def test_accum_state_of_never_visible_rows():
    """carry_in = 0 leaves acc = 0, l = 0 for a row without keys and a later
    round merges into it; a carry_in = 1 round that shows a row nothing
    leaves its state bit for bit; finalize of l == 0 gives o = 0,
    lse = -inf."""
    dtype = torch.float16
    c = sr.rect_case(2, 2, 64, dtype)
    P = _P()
    q, k, v, qs, ks = _gpu(c, "q", "k", "v", "q_seg", "kv_seg")
    dead = (c["q_seg"][0] == 9).cuda()
    state = P.fwd_accum(None, q, k, v, c["scale"], False, seg=(qs, ks))
    acc, m, l = (t.clone() for t in state)
    assert (acc[:, dead] == 0).all() and (l[:, :, dead] == 0).all()
    o, lse = P.fwd_finalize(state, dtype)
    assert (o[:, dead] == 0).all() and (lse[:, :, dead] == -math.inf).all()
    assert o.isfinite().all()
    # round 2 shows every row nothing (ids disjoint from all q ids)
    state = P.fwd_accum(state, q, k, v, c["scale"], False,
                        seg=(qs, torch.full_like(ks, 77)))
    for a, b in zip(state, (acc, m, l)):
        assert torch.equal(a, b)
    # round 3 gives the dead rows keys: they come out as that round alone
    ks3 = torch.full_like(ks, 9)
    state = P.fwd_accum(state, q[:, 90:], k, v, c["scale"], False,
                        row_offset=90, seg=(qs[:, 90:], ks3))
    o3, lse3 = P.fwd_finalize(state, dtype)
    o_ref, lse_ref = sr.seg_fwd(c["q"][:, 90:], c["k"], c["v"], c["scale"],
                                False, c["q_seg"][:, 90:], ks3.cpu())
    gt = gates(dtype, 1)
    torch.testing.assert_close(o3[:, 90:].float().cpu(), o_ref, **gt["o"])
    torch.testing.assert_close(lse3[:, :, 90:].cpu(), lse_ref, **gt["lse"])
    torch.testing.assert_close(o3[:, :90], o[:, :90], rtol=0, atol=0)


# ---- 3. all-equal ids are the id-free call, bit for bit ---------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("d,heads", [(64, (2, 2)), (128, (4, 2))])
@pytest.mark.parametrize("causal", [True, False])
def test_equal_ids_bitwise_equal_no_ids(causal, d, heads, dtype):
    c = sr.causal_case(*heads, d, dtype) if causal else \
        sr.rect_case(*heads, d, dtype)
    q, k, v, do = _gpu(c, "q", "k", "v", "do")
    P = _P()
    seg = (torch.full(q.shape[:2], -5, dtype=torch.int32, device="cuda"),
           torch.full(k.shape[:2], -5, dtype=torch.int32, device="cuda"))
    a = _run(P, q, k, v, do, c["scale"], causal, None)
    b = _run(P, q, k, v, do, c["scale"], causal, seg)
    for name in a:
        assert torch.equal(a[name], b[name]), name


# ---- 4. arbitrary ids ---------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("causal", [True, False])
def test_arbitrary_ids(causal, dtype):
    """A seeded shuffle of a few ids, negative and sparse, non-monotone: the
    pre-pass takes its scan path and the ranges are only a hull."""
    c = dict(sr.causal_case(4, 2, 128, dtype) if causal else
             sr.rect_case(4, 2, 128, dtype))
    g = torch.Generator().manual_seed(5)
    vals = torch.tensor([-7, 0, 3, 1 << 20], dtype=torch.int32)
    sq, sk = c["q"].shape[1], c["k"].shape[1]
    ks = vals[torch.randint(0, 4, (2, sk), generator=g)]
    qs = ks.clone() if causal else vals[torch.randint(0, 4, (2, sq),
                                                      generator=g)]
    c["o"], c["lse"] = sr.seg_fwd(c["q"], c["k"], c["v"], c["scale"], causal,
                                  qs, ks)
    q, k, v, do = _gpu(c, "q", "k", "v", "do")
    got = _run(_P(), q, k, v, do, c["scale"], causal, (qs.cuda(), ks.cuda()))
    _assert_gates(got, _ref_with_kernel_delta(c, got, qs, ks, causal), dtype,
                  2, "seg-arbitrary")


# ---- 5. skipping, shown by function -------------------------------------------

def _plain(b, sq, sk, n, nk, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b, sq, n, d, generator=g).to(dtype),
            torch.randn(b, sk, nk, d, generator=g).to(dtype),
            torch.randn(b, sk, nk, d, generator=g).to(dtype),
            torch.randn(b, sq, n, d, generator=g).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("d", [64, 128])
def test_fwd_dq_skip_invisible_kv_tiles(d, dtype):
    """Queries all id 0; keys id 0 for two tiles, id 1 after, and the id-1
    K/V rows NaN: a loaded tile would poison o, lse and dq through 0 * NaN."""
    sq, sk, n, nk = 320, 384, 4, 2
    q, k, v, do = _plain(2, sq, sk, n, nk, d, dtype, 11 + d)
    qs = torch.zeros(2, sq, dtype=torch.int32)
    ks = torch.zeros(2, sk, dtype=torch.int32)
    ks[:, 128:] = 1
    sc = 1.0 / math.sqrt(d)
    o_ref, lse_ref = sr.seg_fwd(q, k[:, :128], v[:, :128], sc, False, qs,
                                ks[:, :128])
    kn, vn = k.clone(), v.clone()
    kn[:, 128:] = math.nan
    vn[:, 128:] = math.nan
    P = _P()
    o, lse = P.fwd(q.cuda(), kn.cuda(), vn.cuda(), sc, False,
                   seg=(qs.cuda(), ks.cuda()))
    delta = P.bwd_preprocess(o.to(dtype), do.cuda())
    dq = torch.zeros(2, sq, n, d, device="cuda")
    dk = torch.zeros(2, sk, nk, d, device="cuda")
    dv = torch.zeros_like(dk)
    P.bwd_accum(do.cuda(), q.cuda(), kn.cuda(), vn.cuda(), delta, lse, sc,
                False, False, dq, dk, dv, seg=(qs.cuda(), ks.cuda()))
    assert o.isfinite().all() and lse.isfinite().all() and dq.isfinite().all()
    c = dict(q=q, k=k[:, :128], v=v[:, :128], do=do, lse=lse_ref, scale=sc)
    ref = _ref_with_kernel_delta(dict(c, o=o_ref), {"o": o}, qs, ks[:, :128],
                                 False)
    gt = gates(dtype, 2)
    torch.testing.assert_close(o.cpu(), o_ref, **gt["o"])
    torch.testing.assert_close(lse.cpu(), lse_ref, **gt["lse"])
    torch.testing.assert_close(dq.cpu(), ref["dq"], **gt["dq"])
    # the id-1 keys belong to no query: nothing is added to their rows
    assert (dk[:, 128:] == 0).all() and (dv[:, 128:] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("d,heads", [(64, (2, 2)), (128, (4, 2))])
def test_dkv_skip_invisible_q_tiles(d, heads, dtype):
    """All keys id 0; the id-1 rows of q, dO, lse and delta NaN."""
    sq, sk = 384, 320
    n, nk = heads
    q, k, v, do = _plain(2, sq, sk, n, nk, d, dtype, 23 + d)
    qs = torch.zeros(2, sq, dtype=torch.int32)
    qs[:, 192:] = 1
    ks = torch.zeros(2, sk, dtype=torch.int32)
    sc = 1.0 / math.sqrt(d)
    o_ref, lse_ref = sr.seg_fwd(q[:, :192], k, v, sc, False, qs[:, :192], ks)
    o16 = o_ref.to(dtype).float()
    delta_ref = (o16 * do[:, :192].float()).sum(-1).transpose(1, 2)
    _, dk_ref, dv_ref = sr.seg_bwd(do[:, :192], q[:, :192], k, v, lse_ref, sc,
                                   False, qs[:, :192], ks, delta=delta_ref)
    qn, don = q.clone(), do.clone()
    qn[:, 192:] = math.nan
    don[:, 192:] = math.nan
    lse = torch.full((2, n, sq), math.nan)
    delta = torch.full((2, n, sq), math.nan)
    lse[:, :, :192], delta[:, :, :192] = lse_ref, delta_ref
    dq = torch.zeros(2, sq, n, d, device="cuda")
    dk = torch.zeros(2, sk, nk, d, device="cuda")
    dv = torch.zeros_like(dk)
    _P().bwd_accum(don.cuda(), qn.cuda(), k.cuda(), v.cuda(), delta.cuda(),
                   lse.cuda(), sc, False, False, dq, dk, dv,
                   seg=(qs.cuda(), ks.cuda()))
    assert dk.isfinite().all() and dv.isfinite().all()
    gt = gates(dtype, n // nk)
    torch.testing.assert_close(dk.cpu(), dk_ref, **gt["dk"])
    torch.testing.assert_close(dv.cpu(), dv_ref, **gt["dv"])


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_element_mask_gives_exactly_zero_weight(dtype):
    """A boundary inside a subtile (kv 100) with large finite poison behind
    it: the outputs are bitwise those of the same call with zeros in the
    poison's place, and within the gates of the reference."""
    d, sq, sk, n, nk = 128, 320, 320, 4, 2
    q, k, v, do = _plain(2, sq, sk, n, nk, d, dtype, 77)
    qs = torch.zeros(2, sq, dtype=torch.int32)
    ks = torch.zeros(2, sk, dtype=torch.int32)
    ks[:, 100:] = 1
    sc = 1.0 / math.sqrt(d)
    P = _P()
    outs = []
    for kfill, vfill in ((0.0, 0.0), (60.0, 3.0e4)):
        kp, vp = k.clone(), v.clone()
        kp[:, 100:] = kfill
        vp[:, 100:] = vfill
        outs.append(_run(P, q.cuda(), kp.cuda(), vp.cuda(), do.cuda(), sc,
                         False, (qs.cuda(), ks.cuda())))
    for name in ("o", "lse", "dq"):
        assert torch.equal(outs[0][name], outs[1][name]), name
    for name in ("dk", "dv"):
        assert torch.equal(outs[0][name][:, :100], outs[1][name][:, :100])
        assert (outs[1][name][:, 100:] == 0).all(), name
    o_ref, lse_ref = sr.seg_fwd(q, k, v, sc, False, qs, ks)
    gt = gates(dtype, 2)
    torch.testing.assert_close(outs[1]["o"].cpu(), o_ref, **gt["o"])
    torch.testing.assert_close(outs[1]["lse"].cpu(), lse_ref, **gt["lse"])


def _ranges(ws, b, sq, sk):
    """(q block ranges over kv tiles, kv block ranges over q tiles) from the
    pre-pass workspace (word layout: include/burst_attn_hip.h)."""
    tq, tk, bq, bk = -(-sq // 64), -(-sk // 64), -(-sq // 256), -(-sk // 256)
    ws = ws.cpu()
    o = 2 * b + 2 * b * tk
    qr = ws[o:o + 2 * b * bq].view(b, bq, 2)
    o += 2 * b * bq + 2 * b * tq
    return qr, ws[o:o + 2 * b * bk].view(b, bk, 2)


def _sharing(own, strm):
    """Per 256-row block of `own`, the 64-row tiles of `strm` that share an
    id with it ([B] lists of sets)."""
    out = []
    for ob, sb in zip(own, strm):
        out.append([{t for t in range(-(-len(sb) // 64))
                     if set(sb[64 * t:64 * t + 64].tolist())
                     & set(ob[i:i + 256].tolist())}
                    for i in range(0, len(ob), 256)])
    return out


def test_prepass_ranges():
    """Non-decreasing ids: a block's range is exactly the tiles that share
    an id with it.  Arbitrary ids: it contains them."""
    from burst_attn_amd._ext import load_extension

    ext = load_extension()
    mono = sr.ids_from_cu(sr.CAUSAL_CU, sr.CAUSAL_S)
    g = torch.Generator().manual_seed(9)
    mixed = torch.randint(-3, 4, (700,), generator=g).to(torch.int32)
    sparse = mixed.clone()
    sparse[:] = 5
    sparse[300:340] = -2
    for q_ids, k_ids, exact in ((mono, mono, True),
                                (mono, torch.cat([mono, mono + 7]), True),
                                (mixed, mixed, False),
                                (sparse, sparse.flip(0), False)):
        qs = torch.stack([q_ids, q_ids + 1]).cuda()
        ks = torch.stack([k_ids, k_ids + 1]).cuda()
        ws = ext.attn_seg_prepass(qs, ks)
        qr, kr = _ranges(ws, 2, qs.shape[1], ks.shape[1])
        for rng, want in ((qr, _sharing(qs.cpu(), ks.cpu())),
                          (kr, _sharing(ks.cpu(), qs.cpu()))):
            for b in range(2):
                for blk, tiles in enumerate(want[b]):
                    lo, hi = rng[b, blk].tolist()
                    got = set(range(lo, hi))
                    assert tiles <= got, (b, blk, lo, hi, tiles)
                    if exact:
                        assert got == tiles, (b, blk, lo, hi, tiles)


# ---- 6. ring replay -----------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("layout", ["zigzag", "striped"])
@pytest.mark.parametrize("W", [3, 4])
def test_ring_replay(W, layout, d, dtype):
    c = srr.ring_case(W, d, dtype)
    q, k, v, do, ids = _gpu(c, "q", "k", "v", "do", "q_seg")
    got = srr.replay_ring_seg(_P(), q, k, v, do, ids, W, c["scale"], True,
                              layout)
    got = dict(zip(("o", "lse", "dq", "dk", "dv"), got))
    # the ring's delta is rowsum(o in the input dtype * dO) over whole rows
    _assert_gates(got, _ref_with_kernel_delta(c, got, c["q_seg"], c["kv_seg"],
                                              True),
                  dtype, srr.N // srr.NK, f"seg-ring-{layout}-W{W}-d{d}")


# ---- 7. rejected knobs ----------------------------------------------------------

@pytest.mark.parametrize("knob,value,which", [
    ("BA_FWD_SUBT", "0", "fwd"), ("BA_FWD_VPATH", "1", "fwd"),
    ("BA_FWD_NBUF", "4", "fwd"), ("BA_FWD_NT", "256", "fwd"),
    ("BA_FWD_KREG", "1", "fwd"), ("BA_BWD_FUSED", "1", "bwd"),
    ("BA_BWD_FUSED", "2", "bwd"), ("BA_BWD_DK_FLIP", "1", "bwd"),
    ("BA_DQ_PIPE", "1", "bwd")])
def test_unsupported_knobs_raise_with_ids(monkeypatch, knob, value, which):
    c = sr.rect_case(2, 2, 64, torch.float16)
    q, k, v, do, qs, ks = _gpu(c, "q", "k", "v", "do", "q_seg", "kv_seg")
    P = _P()
    lse, delta = c["lse"].cuda(), torch.zeros_like(c["lse"]).cuda()
    dq = torch.zeros(q.shape, device="cuda")
    dk = torch.zeros(k.shape, device="cuda")
    dv = torch.zeros_like(dk)
    monkeypatch.setenv(knob, value)
    with pytest.raises(RuntimeError, match=f"{knob}={value}.*segment ids"):
        if which == "fwd":
            P.fwd(q, k, v, c["scale"], False, seg=(qs, ks))
        else:
            P.bwd_accum(do, q, k, v, delta, lse, c["scale"], False, False, dq,
                        dk, dv, seg=(qs, ks))
    torch.cuda.synchronize()
    assert (dq == 0).all() and (dk == 0).all() and (dv == 0).all()
    if which == "fwd":
        with pytest.raises(RuntimeError, match=f"{knob}={value}"):
            P.fwd_accum(None, q, k, v, c["scale"], False, seg=(qs, ks))


def test_one_id_tensor_alone_raises():
    c = sr.rect_case(2, 2, 64, torch.float16)
    q, k, v, qs = _gpu(c, "q", "k", "v", "q_seg")
    with pytest.raises(RuntimeError, match="together"):
        _P().fwd(q, k, v, c["scale"], False, seg=(qs, None))


# ---- 8. / 9. BA_FWD_VT and run-to-run determinism --------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_vt_knob_does_not_change_results_with_ids(monkeypatch, dtype):
    c = sr.causal_case(4, 2, 128, dtype)
    q, k, v, do, ids = _gpu(c, "q", "k", "v", "do", "q_seg")
    P = _P()
    outs = []
    for vt in ("0", "1"):
        monkeypatch.setenv("BA_FWD_VT", vt)
        o, lse = P.fwd(q, k, v, c["scale"], True, seg=(ids, ids))
        st = P.fwd_accum(None, q, k, v, c["scale"], True, seg=(ids, ids))
        outs.append((o, lse) + tuple(st))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("heads", HEADS, ids=lambda h: f"n{h[0]}k{h[1]}")
def test_backward_with_ids_is_deterministic(heads, dtype):
    c = sr.causal_case(*heads, 128, dtype)
    q, k, v, do, ids = _gpu(c, "q", "k", "v", "do", "q_seg")
    P = _P()
    a = _run(P, q, k, v, do, c["scale"], True, (ids, ids))
    b = _run(P, q, k, v, do, c["scale"], True, (ids, ids))
    for name in a:
        assert torch.equal(a[name], b[name]), name


# ---- 10. the public API at W = 1 ---------------------------------------------------

@pytest.mark.parametrize("striped", [False, True])
@pytest.mark.parametrize("id_dtype", [torch.int32, torch.int64])
def test_interface_single_rank_with_segment_ids(striped, id_dtype):
    import os

    import torch.distributed as dist

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29713")
        dist.init_process_group("nccl", rank=0, world_size=1)
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    dtype = torch.float16
    c = sr.causal_case(4, 2, 128, dtype)
    q, k, v = (c[n].cuda().requires_grad_() for n in ("q", "k", "v"))
    func = burst_attn_func_striped if striped else burst_attn_func
    o = func(q, k, v, None, "cuda", True,
             segment_ids=c["q_seg"].to(id_dtype).cuda())
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), c["do"].cuda())
    got = {"o": o, "dq": dq, "dk": dk, "dv": dv}
    ref = _ref_with_kernel_delta(c, got, c["q_seg"], c["kv_seg"], True)
    gt = gates(dtype, 2)
    for name, out in got.items():
        torch.testing.assert_close(out.float().cpu(), ref[name], **gt[name])
