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

    def fwd(self, q, k, v, scale, causal, seg=None, band=None):
        q_seg, kv_seg = seg if seg is not None else (None, None)
        return self._ext.attn_fwd(q, k, v, float(scale), bool(causal),
                                  q_seg, kv_seg, **self._band_kw(band))

    def bwd_preprocess(self, o, do, out=None):
        return self._ext.attn_bwd_preprocess(o, do, out)

    def bwd(self, do, q, k, v, delta, lse, scale, causal, deterministic,
            seg=None, band=None):
        q_seg, kv_seg = seg if seg is not None else (None, None)
        return self._ext.attn_bwd(
            do, q, k, v, delta, lse, float(scale), bool(causal),
            bool(deterministic), q_seg, kv_seg, **self._band_kw(band),
        )

    def bwd_accum(self, do, q, k, v, delta, lse, scale, causal, deterministic,
                  dq, dk, dv, seg=None, band=None):
        q_seg, kv_seg = seg if seg is not None else (None, None)
        self._ext.attn_bwd_accum(
            do, q, k, v, delta, lse, float(scale), bool(causal),
            bool(deterministic), dq, dk, dv, q_seg, kv_seg,
            **self._band_kw(band),
        )

    def merge(self, o, lse, o_i, lse_i):
        return _merge_scale_out_lse(o, lse, o_i, lse_i)

    # ---- carry-in accumulator path (in-kernel LSE merge; lao.py design) --
    # state = (acc fp32 [B,S,N,D] unnormalised O, m fp32 [B,N,S] exp2-domain
    # running max, l fp32 [B,N,S] running sum) over the rank's FULL chunk;
    # row_offset targets the zigzag-half / striped-shift row windows.
    def fwd_accum(self, state, q, k, v, scale, causal, row_offset=0, seg=None,
                  band=None):
        # the .s-built module carries the D=128 production variants only,
        # and no segment or band form: with either the in-binary kernel runs
        if (self._asm_fwd and q.shape[3] == 128 and seg is None
                and band is None):
            accum = self._ext.attn_fwd_accum_asm
        elif seg is not None or band is not None:
            q_seg, kv_seg = seg if seg is not None else (None, None)
            accum = functools.partial(self._ext.attn_fwd_accum,
                                      q_seg=q_seg, kv_seg=kv_seg,
                                      **self._band_kw(band))
        else:
            accum = self._ext.attn_fwd_accum
        if state is None:
            assert row_offset == 0, "state is created by a full-row round"
            B, S, N, D = q.shape
            acc = torch.empty(B, S, N, D, dtype=torch.float32, device=q.device)
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

    def fwd_empty_state(self, q):
        """The state of "no key seen yet" over q's [B, S, N, D] rows."""
        B, S, N, D = q.shape
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
