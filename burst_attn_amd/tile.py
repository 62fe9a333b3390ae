"""Local flash-attention tile layer — the HIP/CDNA4 compute path.

This is the layer that replaces the reference's three interchangeable
backends (flash-attn CUDA extension / Triton ``lao.py`` / pure-torch math,
dispatched at ``burst_attn/burst_utils.py:103-249``) with ONE hand-written
gfx950 HIP kernel pair (north_star: no Triton, no flash-attn extension,
no multi-backend dispatch).

Provider contract (all tensors in flash layout [B, S, N, D]; lse/delta in
[B, N, S] fp32 — the layouts the flash-attn extension hands the reference,
``burst_utils.py:149-177``):

  fwd(q, k, v, scale, causal)            -> (o_i fp32 [B,Sq,N,D],
                                             lse_i fp32 [B,N,Sq])
  bwd_preprocess(o, do, out=None)        -> delta fp32 [B,N,S]
                                            (= rowsum(o*do); the flash bwd
                                            preprocess, cf. lao.py:247-269)
  bwd(do, q, k, v, delta, lse, scale,
      causal, deterministic)             -> (dq fp32 [.,.,N,D],
                                             dk, dv fp32 [.,.,Nk,D])
  bwd_accum(do, q, k, v, delta, lse,
      scale, causal, deterministic,
      dq, dk, dv)                        -> None; ADDS the tile's dq/dk/dv
                                            contribution into the given
                                            fp32 accumulators (strided
                                            views allowed) — the ring's
                                            round accumulation runs in the
                                            kernel epilogues, not python
                                            adds
  merge(o, lse, o_i, lse_i)              -> merged (o, lse); o [B,S,N,D]
                                            fp32, lse [B,S,N,1] fp32,
                                            per burst_utils.py:20-33.

Head convention (grouped-query attention): q, do, o, dq and the fwd_accum
state carry N heads; k, v, dk, dv carry Nk heads with N % Nk == 0.  Query
head h attends KV head h // G, G = N // Nk (the flash-attn convention);
dk/dv are the sum over the G query heads of each group; lse and delta
stay per query head ([B, N, S]).  Nk == N is plain multi-head attention.
No signature carries G: the shapes do.

Segment ids (packed sequences): ``fwd``, ``fwd_accum``, ``bwd`` and
``bwd_accum`` take an optional keyword ``seg=(q_seg, kv_seg)``, two int32
tensors ``[B, Sq]`` and ``[B, Sk]`` with a contiguous last dim, on q's
device.  Pair (q row i, kv row j) is then visible iff
``q_seg[b, i] == kv_seg[b, j]``, on top of ``causal``; no id value is
special.  The ids belong to the rows actually passed: ``fwd_accum`` slices
nothing itself, its caller hands in the windowed views that match its
windowed q and k/v.  A row that sees no key gives ``o = 0``, ``lse = -inf``
and zero gradients.  A caller without ids passes no ``seg`` keyword at all,
so a provider that predates it keeps working for id-free calls.

Bands (sliding windows): the same four methods take an optional keyword
``band=(lo, hi)``, two Python ints.  Pair (q row i, kv row j) *of the
tensors passed* is then visible iff ``lo <= i - j <= hi``.  Rectangular
tiles (``Sq != Sk``) are allowed, ``lo`` may be negative and either bound
may be huge.  With ``causal=True`` the band is cut at the diagonal
(``lo = max(lo, 0)``) and ``Sq == Sk`` is still demanded.  ``lo > hi`` is a
caller bug and an error.  A row that sees no key behaves as with ids: the
stateless forward gives ``o = 0``, ``lse = -inf``, a carry-in call leaves the
row's state untouched, the backward adds exactly zero from and to it.
``band`` and ``seg`` together are refused.  A caller without a band passes
no ``band`` keyword at all.  ``fwd_empty_state(q)`` returns the carry-in
state of "no key seen yet" over the rank's full ``[B, S, N, D]`` q:
finalizing it gives ``o = 0``, ``lse = -inf``, and ``fwd_accum`` merges into
it at any ``row_offset``; a ring whose first tile does not cover every row
starts from it.

Logit soft-capping: the same four methods take an optional keyword
``softcap``, a positive Python float.  Every score ``s = q.k * scale`` then
becomes ``softcap * tanh(s / softcap)`` before the softmax; ``causal`` applies
as without it, ``lse`` is the log-sum-exp of the capped scores, and the state
of ``fwd_accum`` keeps its contract, so rounds merge as long as every round
of a ring passes the same value.  ``None`` (and ``0.0``, the flash-attn
"off") is the call without it.  ``softcap`` with ``seg`` or ``band`` is
refused.  A caller without a cap passes no ``softcap`` keyword at all.

Block masks (block-sparse attention): the same four methods take an optional
keyword ``blocks=(mask2d, BS)``: a ``uint8`` tensor
``[Bm, Hm, ceil(Sq/BS), ceil(Sk/BS)]`` on q's device, any strides (a view is
handed to the kernel side by its element strides, nothing is copied), and the
block size, a power of two >= 64.  ``Bm`` is 1 or ``B``, ``Hm`` 1 or ``Nk``:
one row of blocks per KV head, shared by the query heads of its group.  Pair
(q row i, kv row j) *of the tensors passed* is then visible iff
``mask2d[b, h // G, i // BS, j // BS]`` is nonzero, on top of ``causal``
(which keeps demanding ``Sq == Sk``).  The kernels walk lists of the set
blocks' tiles, so work follows the number of set blocks.  A row that sees no
key behaves as with ids.  ``blocks`` with ``seg``, ``band`` or ``softcap`` is
refused.  A caller without a mask passes no ``blocks`` keyword at all.

Unequal widths (multi-head latent attention heads): q and k ``[.., 192]``
with v ``[.., 128]`` run a kernel set of their own through the same methods,
with no keyword: the v width is read from v.  o, do, the ``fwd_accum``
accumulator and dv are then 128 wide, dq and dk 192 wide; ``scale`` is the
caller's (the interface defaults to ``1/sqrt(192)``).  ``fwd_empty_state(q,
v_dim=128)`` sizes its accumulator for it.  ``seg``, ``band``, ``softcap`` and
``blocks`` with this shape are refused.  Any other pair of differing widths
is an error naming both.

FP8 (``torch.float8_e4m3fn`` q, k, v, the gfx950 native OCP e4m3): ``fwd`` and
``fwd_accum`` run a forward of their own on the K = 64 fp8 MFMA and take an
optional keyword ``descale=(sq, sk, sv)``, three positive finite Python
floats: the real values are ``q8 * sq`` and so on, per tensor.  head_dim 128,
equal widths.  o, the state and lse are fp32 in real units exactly as with
16-bit inputs, so ``fwd_empty_state``, ``fwd_finalize`` and ``merge`` are
unchanged.  There is no backward; ``seg``, ``band``, ``softcap`` and
``blocks`` with fp8 are refused.  A caller without fp8 inputs passes no
``descale`` keyword at all.

Block-scaled FP8: ``descale=(dq, dk, dv)`` may instead be three fp32 tensors
on q's device with a contiguous last dim, ``dq [B, N, Sq]`` (one per q row and
head), ``dk [B, Nk, ceil(Sk / 64)]`` (one per 64-row tile of the k passed and
KV head) and ``dv [B, Nk, 128]`` (one per v channel and KV head): real values
``q8 * dq[row]``, ``k8 * dk[tile]``, ``v8 * dv[channel]``, read by the kernel on
the device.  They describe the rows actually passed: the caller slices them as
it slices ``seg``, so a k view starts on a multiple of 64 rows of the tensor
that was quantised.  Views are handed over by their strides.  The state stays
fp32 in real units, so rounds with different scales merge.  A mix of floats
and tensors is refused.  ``quantize_fp8(x, mode)`` (``"row"``, ``"tile"``,
``"channel"``) is the HIP quantiser that produces ``(x8, scale)`` from fp16 or
bf16 ``[B, S, H, 128]``.

ALiBi: ``fwd``, ``fwd_accum``, ``bwd`` and ``bwd_accum`` take an optional
keyword ``alibi=(slopes, offset, stride)``: an fp32 tensor ``[1 or B, N]``,
contiguous, on q's device, with one slope per *query* head, and two Python
ints, ``stride >= 1``.  Pair (q row i, kv row j) *of the tensors passed* then
gets the bias ``-slopes[b, h] * |stride * (i - j) + offset|`` added to its
score ``q.k * scale`` before the softmax; ``causal`` applies as without it and
``lse`` is the log-sum-exp of the biased scores.  The two ints place the
tensors in a longer sequence: a contiguous piece pair has ``stride = 1`` and
``offset = Pq - Pk``, the global positions of their first rows; rows dealt
round-robin to W ranks have ``stride = W``.  The state of ``fwd_accum`` keeps
its contract, so rounds with different offsets merge.  The slopes get no
gradient.  head_dim 64 and 128; ``alibi`` with ``seg``, ``band``,
``softcap``, ``blocks``, unequal widths or fp8 inputs is refused.  A caller
without ALiBi passes no ``alibi`` keyword at all.

The default provider is the gfx950 HIP extension and FAILS LOUDLY if the
extension is missing on a GPU machine — there is no CPU/eager fallback in
the product path.  Tests may inject an oracle-backed provider via
``_set_tile_provider_for_testing`` (test infrastructure only).
"""

import functools

import torch

__all__ = ["get_tile_provider", "_set_tile_provider_for_testing", "HipTileProvider"]


@torch.jit.script
def _merge_scale_out_lse(o, lse, o_i, lse_i):
    # restates cuda_scale_out_lse_helper (reference burst_utils.py:20-33)
    o_i = o_i.to(torch.float32)
    lse_i = lse_i.transpose(-2, -1).unsqueeze(-1).contiguous()
    new_lse = lse + torch.log1p(torch.exp(lse_i - lse))
    o = torch.exp(lse - new_lse) * o + torch.exp(lse_i - new_lse) * o_i
    return o, new_lse


class HipTileProvider:
    """gfx950 HIP kernels behind the C-ABI in include/burst_attn_hip.h."""

    def __init__(self):
        import json
        import os

        from . import _ext

        self._ext = _ext.load_extension()  # raises loudly if missing
        # BA_FWD_ASM: route fwd_accum through a .s-built hsaco.
        #   1 = the unmodified re-assembly (parity check of the module path)
        #   2 = the hand-scheduled variant (tools/s_patch.py transforms)
        self._asm_fwd = False
        asm = os.environ.get("BA_FWD_ASM", "0")
        if asm in ("1", "2"):
            here = os.path.dirname(os.path.abspath(__file__))
            name = "_asm_fwd.hsaco" if asm == "1" else "_asm_fwd_p.hsaco"
            with open(os.path.join(here, "_asm_fwd_syms.json")) as f:
                syms = json.load(f)
            self._ext.attn_fwd_asm_load(os.path.join(here, name),
                                        syms["f16_accum"],
                                        syms["bf16_accum"])
            self._asm_fwd = True

    @staticmethod
    def _band_kw(band):
        """The extension's keywords of a ``band=(lo, hi)``; none without."""
        if band is None:
            return {}
        lo, hi = band
        return {"band_lo": int(lo), "band_hi": int(hi)}

    @staticmethod
    def _cap_kw(softcap, seg, band):
        """The extension's keyword of a ``softcap``; none without one."""
        if softcap is None or softcap == 0.0:
            return {}
        if seg is not None or band is not None:
            raise RuntimeError(
                "softcap and " + ("seg" if seg is not None else "band")
                + " are not supported together yet")
        return {"softcap": float(softcap)}

    @staticmethod
    def _blk_kw(blocks, seg, band, softcap):
        """The extension's keywords of a ``blocks=(mask2d, BS)``; none
        without."""
        if blocks is None:
            return {}
        other = ("seg" if seg is not None else "band" if band is not None
                 else "softcap" if softcap else None)
        if other:
            raise RuntimeError(
                f"blocks and {other} are not supported together yet")
        mask2d, bs = blocks
        return {"block_mask": mask2d, "block_size": int(bs)}

    @staticmethod
    def _alibi_kw(alibi, q, v, seg, band, softcap, blocks):
        """The extension's keywords of an ``alibi=(slopes, offset, stride)``;
        none without."""
        if alibi is None:
            return {}
        other = ("seg" if seg is not None else "band" if band is not None
                 else "softcap" if softcap else "blocks" if blocks is not None
                 else "fp8 inputs" if q.dtype == torch.float8_e4m3fn else None)
        if other:
            raise RuntimeError(
                f"alibi and {other} are not supported together yet")
        if q.shape[3] != v.shape[3]:
            raise RuntimeError(
                f"head_dim pair ({q.shape[3]}, {v.shape[3]}) does not "
                "support alibi (plain calls only)")
        slopes, offset, stride = alibi
        return {"alibi_slopes": slopes, "alibi_offset": int(offset),
                "alibi_stride": int(stride)}

    @staticmethod
    def _check_plain_widths(q, v, seg, band, softcap, blocks):
        """Unequal q/k and v widths have the plain kernel form only."""
        if q.shape[3] == v.shape[3]:
            return
        for name, given in (("seg", seg is not None), ("band", band is not None),
                            ("softcap", bool(softcap)),
                            ("blocks", blocks is not None)):
            if given:
                raise RuntimeError(
                    f"head_dim pair ({q.shape[3]}, {v.shape[3]}) does not "
                    f"support {name} (plain calls only)")

    @staticmethod
    def _fp8_kw(q, descale, seg, band, softcap, blocks):
        """The extension's keyword of an fp8 call; none with 16-bit inputs."""
        if q.dtype != torch.float8_e4m3fn:
            if descale is not None:
                raise RuntimeError(
                    f"descale is for fp8 inputs only, q is {q.dtype}")
            return {}
        for name, given in (("seg", seg is not None), ("band", band is not None),
                            ("softcap", bool(softcap)),
                            ("blocks", blocks is not None)):
            if given:
                raise RuntimeError(
                    f"fp8 inputs do not support {name} (plain calls only)")
        sq, sk, sv = (1.0, 1.0, 1.0) if descale is None else descale
        tensors = [isinstance(x, torch.Tensor) for x in (sq, sk, sv)]
        if all(tensors):  # the block-scaled kernel reads them on the device
            return {"descale": (sq, sk, sv)}
        if any(tensors):
            raise RuntimeError(
                "descale must be three floats or three tensors, not a mix")
        return {"descale": (float(sq), float(sk), float(sv))}

    def fwd(self, q, k, v, scale, causal, seg=None, band=None, softcap=None,
            blocks=None, descale=None, alibi=None):
        al_kw = self._alibi_kw(alibi, q, v, seg, band, softcap, blocks)
        if al_kw:
            return self._ext.attn_fwd(q, k, v, float(scale), bool(causal),
                                      **al_kw)
        self._check_plain_widths(q, v, seg, band, softcap, blocks)
        fp8_kw = self._fp8_kw(q, descale, seg, band, softcap, blocks)
        if fp8_kw:
            return self._ext.attn_fwd(q, k, v, float(scale), bool(causal),
                                      **fp8_kw)
        q_seg, kv_seg = seg if seg is not None else (None, None)
        return self._ext.attn_fwd(q, k, v, float(scale), bool(causal),
                                  q_seg, kv_seg, **self._band_kw(band),
                                  **self._cap_kw(softcap, seg, band),
                                  **self._blk_kw(blocks, seg, band, softcap))

    def bwd_preprocess(self, o, do, out=None):
        return self._ext.attn_bwd_preprocess(o, do, out)

    def bwd(self, do, q, k, v, delta, lse, scale, causal, deterministic,
            seg=None, band=None, softcap=None, blocks=None, alibi=None):
        al_kw = self._alibi_kw(alibi, q, v, seg, band, softcap, blocks)
        if al_kw:
            return self._ext.attn_bwd(
                do, q, k, v, delta, lse, float(scale), bool(causal),
                bool(deterministic), **al_kw)
        self._check_plain_widths(q, v, seg, band, softcap, blocks)
        q_seg, kv_seg = seg if seg is not None else (None, None)
        return self._ext.attn_bwd(
            do, q, k, v, delta, lse, float(scale), bool(causal),
            bool(deterministic), q_seg, kv_seg, **self._band_kw(band),
            **self._cap_kw(softcap, seg, band),
            **self._blk_kw(blocks, seg, band, softcap),
        )

    def bwd_accum(self, do, q, k, v, delta, lse, scale, causal, deterministic,
                  dq, dk, dv, seg=None, band=None, softcap=None, blocks=None,
                  alibi=None):
        al_kw = self._alibi_kw(alibi, q, v, seg, band, softcap, blocks)
        if al_kw:
            self._ext.attn_bwd_accum(
                do, q, k, v, delta, lse, float(scale), bool(causal),
                bool(deterministic), dq, dk, dv, **al_kw)
            return
        self._check_plain_widths(q, v, seg, band, softcap, blocks)
        q_seg, kv_seg = seg if seg is not None else (None, None)
        self._ext.attn_bwd_accum(
            do, q, k, v, delta, lse, float(scale), bool(causal),
            bool(deterministic), dq, dk, dv, q_seg, kv_seg,
            **self._band_kw(band), **self._cap_kw(softcap, seg, band),
            **self._blk_kw(blocks, seg, band, softcap),
        )

    def merge(self, o, lse, o_i, lse_i):
        return _merge_scale_out_lse(o, lse, o_i, lse_i)

    # ---- carry-in accumulator path (in-kernel LSE merge; lao.py design) --
    # state = (acc fp32 [B,S,N,D] unnormalised O, m fp32 [B,N,S] exp2-domain
    # running max, l fp32 [B,N,S] running sum) over the rank's FULL chunk;
    # row_offset targets the zigzag-half / striped-shift row windows.
    def fwd_accum(self, state, q, k, v, scale, causal, row_offset=0, seg=None,
                  band=None, softcap=None, blocks=None, descale=None,
                  alibi=None):
        al_kw = self._alibi_kw(alibi, q, v, seg, band, softcap, blocks)
        self._check_plain_widths(q, v, seg, band, softcap, blocks)
        fp8_kw = self._fp8_kw(q, descale, seg, band, softcap, blocks)
        cap_kw = self._cap_kw(softcap, seg, band)
        blk_kw = self._blk_kw(blocks, seg, band, softcap)
        # the .s-built module carries the D=128 production variants only,
        # and no segment, band, soft-capped or block form: with any of them
        # the in-binary kernel runs
        if al_kw:  # the in-binary ALiBi kernel, never the module kernel
            accum = functools.partial(self._ext.attn_fwd_accum, **al_kw)
        elif fp8_kw:  # a kernel set of its own, never the module kernel
            accum = functools.partial(self._ext.attn_fwd_accum, **fp8_kw)
        elif (self._asm_fwd and q.shape[3] == 128 and v.shape[3] == 128
                and seg is None
                and band is None and not cap_kw and not blk_kw):
            accum = self._ext.attn_fwd_accum_asm
        elif seg is not None or band is not None or cap_kw or blk_kw:
            q_seg, kv_seg = seg if seg is not None else (None, None)
            accum = functools.partial(self._ext.attn_fwd_accum,
                                      q_seg=q_seg, kv_seg=kv_seg,
                                      **self._band_kw(band), **cap_kw,
                                      **blk_kw)
        else:
            accum = self._ext.attn_fwd_accum
        if state is None:
            assert row_offset == 0, "state is created by a full-row round"
            B, S, N, _ = q.shape
            acc = torch.empty(B, S, N, v.shape[3], dtype=torch.float32,
                              device=q.device)
            m = torch.empty(B, N, S, dtype=torch.float32, device=q.device)
            l = torch.empty(B, N, S, dtype=torch.float32, device=q.device)
            accum(q, k, v, float(scale), bool(causal), acc, m, l, False)
            return (acc, m, l)
        acc, m, l = state
        sq = q.shape[1]
        sl = slice(row_offset, row_offset + sq)
        accv, mv, lv = acc[:, sl], m[:, :, sl], l[:, :, sl]
        accum(q, k, v, float(scale), bool(causal), accv, mv, lv, True)
        return state

    def quantize_fp8(self, x, mode):
        """fp16 / bf16 ``[B, S, H, 128]`` -> ``(x8, scale)``: e4m3 and the
        fp32 scales per ``"row"``, 64-row ``"tile"`` or ``"channel"``."""
        return tuple(self._ext.quantize_fp8(x, mode))

    def fwd_empty_state(self, q, v_dim=None):
        """The state of "no key seen yet" over q's [B, S, N, D] rows; the
        accumulator is ``v_dim`` wide where v's width differs from q's."""
        B, S, N, D = q.shape
        D = D if v_dim is None else v_dim
        acc = torch.empty(B, S, N, D, dtype=torch.float32, device=q.device)
        m = torch.empty(B, N, S, dtype=torch.float32, device=q.device)
        l = torch.empty(B, N, S, dtype=torch.float32, device=q.device)
        self._ext.attn_fwd_state_init(acc, m, l)
        return (acc, m, l)

    def fwd_finalize(self, state, out_dtype):
        acc, m, l = state
        return self._ext.attn_fwd_finalize(acc, m, l, out_dtype)


_provider = None
_provider_override = None


def _set_tile_provider_for_testing(provider):
    """TEST INFRASTRUCTURE ONLY — inject a CPU (oracle) tile provider so the
    ring orchestration can be exercised without a GPU.  The product path
    never calls this."""
    global _provider_override
    _provider_override = provider


def get_tile_provider():
    global _provider
    if _provider_override is not None:
        return _provider_override
    if _provider is None:
        _provider = HipTileProvider()
    return _provider
