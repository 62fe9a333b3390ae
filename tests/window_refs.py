"""Reference, inputs and shapes of the sliding-window (band) tests — TEST
INFRASTRUCTURE ONLY; a plain helper shared by the CPU and GPU tests.

The reference is the dense fp64 masked softmax of tests/segment_refs.py
under an explicit mask: ``band_mask`` for a tile call (pair (i, j) of the
tensors passed visible iff ``lo <= i - j <= hi``) and ``global_window_mask``
for a whole sequence (``i - left <= j <= i + right``, -1 unbounded,
``causal`` forcing ``right = 0``).

Edge-needle inputs make one-off band edges visible: q rows have norm
sqrt(d); for each chosen row p the four keys at the two edges of its band,
``p - hi`` and ``p - lo`` (the last visible ones) and ``p - hi - 1`` and
``p - lo + 1`` (the first hidden ones), are hot for q[p] (score about
``a = ln(Sk) + 2``), the visible pair's V rows shifted by +SEG_V_POISON and
the hidden pair's by -SEG_V_POISON.  A band one off at either edge then
moves every output of row p by far more than a gate
(tests/test_window_cpu.py proves it).
"""

import collections
import functools
import math

import torch

from . import segment_refs as sr
from .segment_refs import SEG_V_POISON

B = 2

BandCase = collections.namedtuple("BandCase", "name sq sk lo hi rows d n nk")

# the smallest shapes where the kernels can go wrong: 328 = one full 256-row
# block and a ragged second one, five 64-row tiles and a ragged sixth; the
# rows sit on wave (32), tile (64) and block (256) seams and at the ends
CASES = {
    "a": BandCase("a", 328, 328, 0, 100,
                  (100, 131, 132, 163, 164, 255, 256, 327), 64, 2, 2),
    "b": BandCase("b", 328, 328, -40, 70, (31, 64, 127, 200, 256, 300),
                  128, 4, 2),
    "c": BandCase("c", 96, 320, -250, -130, (0, 31, 32, 63, 64, 95), 64, 4, 2),
    # kv rows above 95 are seen by nobody
    "d": BandCase("d", 96, 320, 0, 40, (), 64, 4, 2),
    # rows 0..199 see nothing
    "e": BandCase("e", 328, 328, 200, 400, (), 64, 2, 2),
}


def band_mask(b, sq, sk, lo, hi):
    """[b, sq, sk] bool: lo <= i - j <= hi."""
    d = torch.arange(sq)[:, None] - torch.arange(sk)[None, :]
    return ((d >= lo) & (d <= hi)).expand(b, -1, -1)


def global_window_mask(S, left, right, causal):
    """[S, S] bool over global positions."""
    if causal:
        right = 0
    d = torch.arange(S)[:, None] - torch.arange(S)[None, :]   # i - j
    m = torch.ones(S, S, dtype=torch.bool)
    if left >= 0:
        m &= d <= left
    if right >= 0:
        m &= d >= -right
    return m


def needle_inputs(b, sq, sk, n, nk, d, dtype, seed, lo, hi, rows):
    """(q, k, v, do) with the band edges of ``rows`` made hot (see the
    module docstring)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, sq, n, d, generator=g)
    q = q * (math.sqrt(d) / q.norm(dim=-1, keepdim=True))
    k = torch.randn(b, sk, nk, d, generator=g)
    v = torch.randn(b, sk, nk, d, generator=g)
    do = torch.randn(b, sq, n, d, generator=g)
    a = math.log(max(sk, 2)) + 2.0
    qh = q[:, :, :: n // nk]
    for p in rows:
        for j, sign in ((p - hi, 1.0), (p - lo, 1.0), (p - hi - 1, -1.0),
                        (p - lo + 1, -1.0)):
            if 0 <= j < sk:
                k[:, j] += (a / math.sqrt(d)) * qh[:, p]
                v[:, j] += sign * SEG_V_POISON
    return tuple(t.to(dtype) for t in (q, k, v, do))


def with_ref(q, k, v, do, mask):
    """The case dict of tests/segment_refs._with_ref under an explicit mask
    ([B, Sq, Sk] bool)."""
    sc = 1.0 / math.sqrt(q.shape[-1])
    o, lse = sr.seg_fwd(q, k, v, sc, False, None, None, mask=mask)
    dq, dk, dv = sr.seg_bwd(do, q, k, v, lse, sc, False, None, None, o=o,
                            mask=mask)
    return dict(q=q, k=k, v=v, do=do, mask=mask, scale=sc, o=o, lse=lse,
                dq=dq, dk=dk, dv=dv)


def band_ref(c, lo, hi):
    """(o, lse, dq, dk, dv) of case dict ``c``'s inputs under another band."""
    mask = band_mask(c["q"].shape[0], c["q"].shape[1], c["k"].shape[1], lo, hi)
    r = with_ref(c["q"], c["k"], c["v"], c["do"], mask)
    return {nm: r[nm] for nm in ("o", "lse", "dq", "dk", "dv")}


@functools.lru_cache(maxsize=None)
def band_case(name, n, nk, d, dtype):
    """Inputs and reference of case ``name`` at the given heads, head_dim
    and dtype; computed once, shared, never modified."""
    c = CASES[name]
    q, k, v, do = needle_inputs(B, c.sq, c.sk, n, nk, d, dtype,
                                9000 + ord(name) + n + d, c.lo, c.hi, c.rows)
    out = with_ref(q, k, v, do, band_mask(B, c.sq, c.sk, c.lo, c.hi))
    out["band"] = (c.lo, c.hi)
    return out


def table_case(name, dtype):
    """Case ``name`` at the heads and head_dim its table row names."""
    c = CASES[name]
    return band_case(name, c.n, c.nk, c.d, dtype)
