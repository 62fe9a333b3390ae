"""GPU tests of the V^T image path of the forward (BA_FWD_VT).

The pre-pass writes V transposed per 64-row kv tile once per call
(layout: burst_attn_amd/csrc/vt_image.h) and the forward kernel copies
those tiles into LDS instead of transposing V itself.  The MFMA operands
are the same bits in the same order either way, so everything here is
torch.equal, never a tolerance: the image against a torch permutation of
V, and the image path's outputs against the in-kernel transpose.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]


def _ext():
    from burst_attn_amd._ext import load_extension

    return load_extension()


def _rand(b, s, n, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, s, n, d, generator=g).to(dtype).cuda()


def _image_ref(v):
    """zero-padded V as [B, T, 64, Nk, D], permuted to [B, Nk, T, D, 64]"""
    b, sk, nk, d = v.shape
    t = (sk + 63) // 64
    pad = torch.zeros(b, t * 64, nk, d, dtype=v.dtype, device=v.device)
    pad[:, :sk] = v
    return pad.reshape(b, t, 64, nk, d).permute(0, 3, 1, 4, 2).contiguous()


@pytest.mark.parametrize("view", ["plain", "striped", "upper_half"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("sk", [1, 63, 64, 65, 296])
def test_vt_image(sk, d, dtype, view):
    """attn_vt_image into a NaN-filled out: every element written, the pad
    columns zero, strided sources read through their strides."""
    b, nk = 2, 2
    if view == "plain":
        v = _rand(b, sk, nk, d, dtype, 300 + sk)
    elif view == "striped":
        v = _rand(b, 2 * sk, nk, d, dtype, 400 + sk)[:, 1::2]
    else:
        v = _rand(b, 2 * sk + 8, nk, d, dtype, 500 + sk)[:, sk + 8:]
    assert v.shape[1] == sk
    t = (sk + 63) // 64
    out = torch.full((b, nk, t, d, 64), float("nan"), dtype=dtype,
                     device="cuda")
    img = _ext().attn_vt_image(v, out)
    assert img.data_ptr() == out.data_ptr()
    assert torch.equal(img, _image_ref(v))
    # and the allocating form
    assert torch.equal(_ext().attn_vt_image(v), img)


@pytest.mark.parametrize("dtype", DTYPES)
def test_too_small_workspace_is_refused_before_launch(dtype):
    """A flat `out` goes to the C entry with its true size.  One element
    short of the image, the launcher returns BAHIP_ERR_WORKSPACE and
    launches nothing: the call raises and the NaN-filled buffer is
    untouched.  With exactly enough, the same buffer receives the image."""
    b, sk, nk, d = 2, 65, 2, 64
    v = _rand(b, sk, nk, d, dtype, 330)
    need = b * nk * 2 * d * 64
    ws = torch.full((need,), float("nan"), dtype=dtype, device="cuda")
    with pytest.raises(RuntimeError, match="workspace"):
        _ext().attn_vt_image(v, ws[:need - 1])
    torch.cuda.synchronize()
    assert torch.isnan(ws).all()
    with pytest.raises(RuntimeError, match="workspace"):
        _ext().attn_vt_image(v, ws[:0])
    img = _ext().attn_vt_image(v, ws)
    assert img.data_ptr() == ws.data_ptr()
    assert torch.equal(img, _image_ref(v))


# Both paths give the same bits, so nothing below can tell from the outputs
# which kernel ran: a forward that quietly kept the in-kernel transpose
# would pass.  What these tests can see is the launcher's decision (the
# workspace size the call allocates, nonzero only where the image form is
# chosen); that the VSRC=1 kernel and the pre-pass are what is then
# launched is shown by the kernel names in the profiler output kept in
# profiles/fwd_vt/.
def _both_forms(q, ka, va, kb, vb, scale, causal):
    """o, lse of the stateless tile on (ka, va); acc, m, l of a fresh
    accumulator on (ka, va) followed by a carry-in call on (kb, vb)"""
    ext = _ext()
    o, lse = ext.attn_fwd(q, ka, va, scale, causal)
    b, sq, n, d = q.shape
    acc = torch.empty(b, sq, n, d, dtype=torch.float32, device=q.device)
    m = torch.empty(b, n, sq, dtype=torch.float32, device=q.device)
    l = torch.empty(b, n, sq, dtype=torch.float32, device=q.device)
    ext.attn_fwd_accum(q, ka, va, scale, causal, acc, m, l, False)
    ext.attn_fwd_accum(q, kb, vb, scale, False, acc, m, l, True)
    return o, lse, acc, m, l


# (B, N, Nk, Sq, Sk, causal, strided V)
PATH_CASES = (
    [(2, 4, 2, sq, sk, False, False)
     for sq, sk in [(296, 296), (64, 1), (300, 63), (257, 65), (512, 128)]]
    + [(2, 4, 2, s, s, True, False) for s in (296, 65, 512)]
    + [(2, 4, 2, 296, 296, False, True),    # striped V (and K) views
       (2, 3, 3, 296, 296, False, False)]   # MHA
)


def _path_inputs(case, d, dtype):
    b, n, nk, sq, sk, causal, strided = case
    q = _rand(b, sq, n, d, dtype, 600)
    if strided:
        ka, va, kb, vb = (_rand(b, 2 * sk, nk, d, dtype, 601 + i)[:, 1::2]
                          for i in range(4))
    else:
        ka, va, kb, vb = (_rand(b, sk, nk, d, dtype, 601 + i)
                          for i in range(4))
    return q, ka, va, kb, vb, 1.0 / math.sqrt(d), causal


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize(
    "case", PATH_CASES,
    ids=["-".join(str(int(x)) for x in c) for c in PATH_CASES])
def test_image_path_equals_in_kernel_transpose(case, d, dtype, monkeypatch):
    """BA_FWD_VT=0 against =1, in-process: o, lse of attn_fwd, and acc, m,
    l of a fresh attn_fwd_accum followed by a carry-in one on a second kv
    chunk, all bitwise equal."""
    args = _path_inputs(case, d, dtype)
    monkeypatch.setenv("BA_FWD_VT", "0")
    old = _both_forms(*args)
    monkeypatch.setenv("BA_FWD_VT", "1")
    b, n, nk, sq, sk = case[:5]
    assert _ext().attn_fwd_workspace_bytes(b, sq, sk, n, nk, d) > 0
    new = _both_forms(*args)
    for name, a, c in zip(("o", "lse", "acc", "m", "l"), old, new):
        assert not torch.isnan(c).any(), name
        assert torch.equal(a, c), name


def _threshold_shapes():
    """(Sq, N, Nk) with ceil(Sq/256) * G one below the auto threshold and
    at it, found from the workspace query itself (N = Nk = 2, so G = 1)"""
    ext = _ext()
    tiles = 1
    while ext.attn_fwd_workspace_bytes(1, 256 * tiles, 64, 2, 2, 128) == 0:
        tiles += 1
        assert tiles <= 4096, "the auto rule never takes the image"
    return tiles


@pytest.mark.parametrize("dtype", DTYPES)
def test_auto_rule_matches_forced_paths(dtype, monkeypatch):
    """With BA_FWD_VT unset a shape below the threshold takes the in-kernel
    transpose and one at it the image (seen through the workspace the call
    allocates), each with the bits of the corresponding forced path.  The
    same reuse count reached through G (grouped heads) decides the same."""
    ext = _ext()
    monkeypatch.delenv("BA_FWD_VT", raising=False)
    thr = _threshold_shapes()
    d, sk = 128, 129
    shapes = [(256 * thr, 2, 2, True)]
    if thr > 1:
        shapes.append((256 * (thr - 1), 2, 2, False))
        # thr - 1 tiles of q rows times G = 2 is at or above the threshold
        # once 2 (thr - 1) >= thr
        shapes.append((256 * (thr - 1), 4, 2, 2 * (thr - 1) >= thr))
    for sq, n, nk, takes_image in shapes:
        monkeypatch.delenv("BA_FWD_VT", raising=False)
        ws = ext.attn_fwd_workspace_bytes(1, sq, sk, n, nk, d)
        assert (ws > 0) == takes_image, (sq, n, nk)
        if takes_image:
            assert ws == 1 * nk * ((sk + 63) // 64) * d * 64 * 2
        q = _rand(1, sq, n, d, dtype, 700)
        k = _rand(1, sk, nk, d, dtype, 701)
        v = _rand(1, sk, nk, d, dtype, 702)
        scale = 1.0 / math.sqrt(d)
        auto = ext.attn_fwd(q, k, v, scale, False)
        monkeypatch.setenv("BA_FWD_VT", "1" if takes_image else "0")
        forced = ext.attn_fwd(q, k, v, scale, False)
        for a, f in zip(auto, forced):
            assert torch.equal(a, f)


def test_experiment_variant_keeps_in_kernel_transpose(monkeypatch):
    """any non-default BA_FWD_* knob selects its experiment variant, which
    has no image form: no workspace even with BA_FWD_VT=1"""
    ext = _ext()
    monkeypatch.setenv("BA_FWD_VT", "1")
    assert ext.attn_fwd_workspace_bytes(1, 512, 512, 2, 2, 128) > 0
    monkeypatch.setenv("BA_FWD_NBUF", "4")
    assert ext.attn_fwd_workspace_bytes(1, 512, 512, 2, 2, 128) == 0
    q = _rand(1, 300, 2, 128, torch.float16, 710)
    o_alt, _ = ext.attn_fwd(q, q, q, 0.1, False)
    monkeypatch.delenv("BA_FWD_NBUF")
    o_img, _ = ext.attn_fwd(q, q, q, 0.1, False)
    # same arithmetic in the same order (profiles/fwd_kernel/README.md)
    assert torch.equal(o_alt, o_img)


@pytest.mark.parametrize("bad", ["2", "-1", "on"])
def test_bad_knob_value_raises_with_its_name(bad, monkeypatch):
    ext = _ext()
    q = _rand(1, 64, 2, 64, torch.float16, 720)
    monkeypatch.setenv("BA_FWD_VT", bad)
    with pytest.raises(RuntimeError, match="BA_FWD_VT"):
        ext.attn_fwd(q, q, q, 0.125, False)
    acc = torch.empty(1, 64, 2, 64, dtype=torch.float32, device="cuda")
    m = torch.empty(1, 2, 64, dtype=torch.float32, device="cuda")
    l = torch.empty_like(m)
    with pytest.raises(RuntimeError, match="BA_FWD_VT"):
        ext.attn_fwd_accum(q, q, q, 0.125, False, acc, m, l, False)
    monkeypatch.delenv("BA_FWD_VT")
    ext.attn_fwd(q, q, q, 0.125, False)  # and the next call is clean
