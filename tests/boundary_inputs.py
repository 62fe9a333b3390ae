"""Seeded input families that put softmax mass on tile boundaries.

TEST INFRASTRUCTURE ONLY.  With randn inputs a row's softmax mass is spread
over all its keys, so an error confined to one (row, key) pair moves the
output by about 1/S of its size and stays under the parity gates' atol.
The families here keep the gates and change the inputs: a few keys on the
kernels' subtile / tile / workgroup / tail seams (``seam_weighted``) or
every row's own diagonal key (``diag_needle``) carry a large share of the
row's mass, so a predicate that is off by one at such a seam moves the
output by O(0.1 .. 1).  tests/test_gate_sensitivity_cpu.py proves on the
CPU that the gates of tests/test_gpu_parity.py then reject such errors
and still pass legitimate low-precision rounding.

Every family returns CPU tensors in the requested dtype, layout
``[B, S, N, D]``; callers move them to the GPU.
"""

import math
from collections import namedtuple

import torch

__all__ = [
    "DO_GAIN",
    "seam_keys",
    "seam_rows",
    "seam_vector",
    "seam_weighted",
    "diag_needle",
    "poisoned_parent",
    "PoisonedParent",
    "view_of",
    "Case",
    "CASES",
    "KNOB_CASES",
    "make_inputs",
    "round2_kv",
    "DOMINATED_GAIN",
    "DOMINATED_MIN_GAP",
    "DOMINATED_CASES",
    "dominated_kv",
    "case_id",
    "dtype_name",
    "K_POISON",
    "V_POISON",
    "SENTINEL",
]

# dO amplification on the seam rows.  8 put the bf16 rounding emulation at
# 0.72 of the dq gate and 4 at 0.48; 2 keeps every emulated output under
# 0.4 of its gate (tests/test_gate_sensitivity_cpu.py asserts <= 0.5) while
# every backward mutant on this family still scores above 5.
DO_GAIN = 2.0

# poison of the parent buffers outside the views (finite on purpose: the
# contract under test is "nothing outside the view is read or written",
# not how 0 * NaN propagates)
K_POISON = 8.0    # x seam_vector: one leaked row scores ~ 8 sqrt(d) >= 64
V_POISON = 1.0e4  # V and dO rows (finite in fp16)
SENTINEL = -12345.0  # fp32 output parents


def seam_keys(sk):
    """Key positions on the kernels' seams: the 32-row subtile, the 64-row
    kv tile, the 256-row workgroup and the ragged tail."""
    return sorted({j for j in (0, 31, 32, 63, 64, 255, 256, sk - 2, sk - 1)
                   if 0 <= j < sk})


def seam_rows(sq):
    """Query rows on the wave (32), workgroup (256) and tail seams."""
    return sorted({i for i in (0, 31, 32, 255, 256, sq - 2, sq - 1)
                   if 0 <= i < sq})


def seam_vector(d):
    """The fixed +-1 direction shared by every q row and the seam keys.  It
    depends on d alone, so keys drawn with another seed stay aligned with
    the same q (the carry-in tests' second round)."""
    g = torch.Generator().manual_seed(977 + d)
    return torch.randint(0, 2, (d,), generator=g).to(torch.float32) * 2 - 1


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def seam_weighted(b, sq, sk, n, nk, d, dtype, seed, beta=None, gain=DO_GAIN):
    """randn q/k/v/do with q += u and k[J] += (beta / sqrt(d)) u.

    u.u = d, so each key of J = seam_keys(sk) gains +beta in scaled score
    on every row.  beta = ln(sk): one seam key weighs about as much as all
    ordinary keys together.  The randn keys first lose their own component
    along u: left in, it adds a per-key N(0, 1) to every row's score, and
    a seam key that drew -2 there is back to an ordinary key's weight on
    all rows at once (the last row's diagonal key then moved o by only
    1.25 bf16 gates when dropped; without it by 4.4).  do is multiplied by
    `gain` on seam_rows(sq).  Returns (q, k, v, do).
    """
    if beta is None:
        beta = math.log(max(sk, 2))
    g = torch.Generator().manual_seed(seed)
    u = seam_vector(d)
    q = _randn(g, b, sq, n, d)
    k = _randn(g, b, sk, nk, d)
    k -= (k @ u / d).unsqueeze(-1) * u
    v = _randn(g, b, sk, nk, d)
    do = _randn(g, b, sq, n, d)
    q += u
    k[:, seam_keys(sk)] += (beta / math.sqrt(d)) * u
    do[:, seam_rows(sq)] *= gain
    return tuple(t.to(dtype) for t in (q, k, v, do))


def _rows_from(t, shift):
    """out[:, j] = t[:, j + shift]; rows outside the sequence are zero."""
    if shift == 0:
        return t
    out = torch.zeros_like(t)
    s = t.shape[1]
    if abs(shift) < s:
        if shift > 0:
            out[:, :s - shift] = t[:, shift:]
        else:
            out[:, -shift:] = t[:, :s + shift]
    return out


def diag_needle(b, s, n, nk, d, dtype, seed, a=None, c=None, lag=0):
    """Causal family: k_j = eps_j + a q_j / sqrt(d) + c q_{j-1} / sqrt(d).

    q rows are normalised to |q|^2 = d, so score(i, i) = a and
    score(i, i + 1) = c up to the eps and cross terms.  a = ln(s): every
    row's own diagonal key, the last key it may see, holds a large share
    of its mass.  c = 2a: the first super-diagonal key would swamp the row
    if it leaked through the mask.  With grouped heads KV head h is built
    from its group's first query head.  Returns (q, k, v, do).

    With `lag` the hot allowed key sits `lag` tokens behind the row and the
    forbidden one max(lag, 1) ahead of it,
        k_j = eps_j + a q_{j+lag} / sqrt(d) + c q_{j-max(lag,1)} / sqrt(d),
    rows outside the sequence contributing zero.  Chunked over W ring ranks
    those keys belong to another rank: they are the boundary pairs of the
    ring's cross-rank tiles (tests/ring_rounds.py).  lag = 0 is the family
    above, bit for bit.
    """
    if a is None:
        a = math.log(max(s, 2))
    if c is None:
        c = 2.0 * a
    g = torch.Generator().manual_seed(seed)
    q = _randn(g, b, s, n, d)
    q = q * (math.sqrt(d) / q.norm(dim=-1, keepdim=True))
    eps = _randn(g, b, s, nk, d)
    v = _randn(g, b, s, nk, d)
    do = _randn(g, b, s, n, d)
    qh = q[:, :, :: n // nk]  # the group's first query head, [B,S,Nk,D]
    q_hot = _rows_from(qh, lag)
    q_prev = _rows_from(qh, -max(lag, 1))
    k = eps + (a / math.sqrt(d)) * q_hot + (c / math.sqrt(d)) * q_prev
    return tuple(t.to(dtype) for t in (q, k, v, do))


PoisonedParent = namedtuple(
    "PoisonedParent", "parents views out_parents out_views")


def _embed(t, fill, pre, post):
    """[B,S,H,D] -> view of a [2B-1, pre+S+post, H+2, D] parent filled with
    `fill` ([D] or scalar): batch rows 0, 2, .., sequence window
    [pre, pre+S), heads [1, H+1)."""
    b, s, h, d = t.shape
    parent = torch.empty(2 * b - 1, pre + s + post, h + 2, d, dtype=t.dtype)
    parent[:] = fill
    view = parent[::2, pre:pre + s, 1:h + 1]
    view.copy_(t)
    return parent, view


def _out_parent(b, s, h, d, pre, post):
    parent = torch.full((2 * b - 1, pre + s + post, h + 2, d), SENTINEL,
                        dtype=torch.float32)
    return parent, parent[::2, pre:pre + s, 1:h + 1]


def poisoned_parent(q, k, v, do, pre=3, post=5):
    """The same q/k/v/do as strided views into larger poisoned parents.

    Each view starts `pre` rows into the parent's sequence axis, carries
    one extra leading and one extra trailing head, and takes every other
    batch row of the parent — the strides and offsets the ring's slices
    produce, and more.  Outside the views K and Q rows are K_POISON * u,
    V and dO rows V_POISON.

    Also returns fp32 output parents pre-filled with SENTINEL and their
    views: acc/dq [.., N, D], dk/dv [.., Nk, D] and m/l [B', N+2, S'].
    Move `parents` / `out_parents` to the GPU and re-slice them there with
    `view_of`.
    """
    d = q.shape[-1]
    ku = (K_POISON * seam_vector(d)).to(q.dtype)
    parents, views = {}, {}
    for name, t, fill in (("q", q, ku), ("k", k, ku), ("v", v, V_POISON),
                          ("do", do, V_POISON)):
        parents[name], views[name] = _embed(t, fill, pre, post)
    b, sq, n, _ = q.shape
    sk, nk = k.shape[1], k.shape[2]
    out_parents, out_views = {}, {}
    for name, s, h in (("acc", sq, n), ("dq", sq, n), ("dk", sk, nk),
                       ("dv", sk, nk)):
        out_parents[name], out_views[name] = _out_parent(b, s, h, d, pre, post)
    for name in ("m", "l"):
        p = torch.full((2 * b - 1, n + 2, pre + sq + post), SENTINEL,
                       dtype=torch.float32)
        out_parents[name] = p
        out_views[name] = p[::2, 1:n + 1, pre:pre + sq]
    return PoisonedParent(parents, views, out_parents, out_views)


def view_of(parent, like_view, like_parent):
    """The view of `parent` (a copy of `like_parent`, e.g. on the GPU) with
    the geometry `like_view` has in `like_parent`."""
    off = like_view.storage_offset() - like_parent.storage_offset()
    return parent.as_strided(like_view.shape, like_view.stride(),
                             parent.storage_offset() + off)


# ---- the shapes the boundary tests run, shared by the GPU tests and the
# CPU sensitivity proof so that the proof covers exactly what runs

Case = namedtuple("Case", "family b sq sk n nk d causal")

_CAUSAL_S = (328,  # two 256-row workgroups and a ragged 72 = 64 + 8 tail
             296,  # five kv tiles: NBUF=4 wraps
             1, 33, 65)
_NONCAUSAL_SQ_SK = ((328, 328), (296, 296), (96, 320),
                    (40, 1), (40, 31), (40, 33), (40, 63), (40, 65))


def _cases():
    out = []
    for d in (128, 64):
        for n, nk in ((4, 2), (2, 2)):
            for s in _CAUSAL_S:
                out.append(Case("seam_weighted", 2, s, s, n, nk, d, True))
                out.append(Case("diag_needle", 2, s, s, n, nk, d, True))
            for sq, sk in _NONCAUSAL_SQ_SK:
                out.append(Case("seam_weighted", 2, sq, sk, n, nk, d, False))
    return out


CASES = _cases()
# the knob-variant tests: S=328, causal diag_needle and non-causal
# seam_weighted, both head dims (each is its own kernel instantiation)
KNOB_CASES = [c for c in CASES if c.sq == 328
              and (c.family == "diag_needle") == c.causal]


def make_inputs(case, dtype, seed_offset=0):
    """(q, k, v, do) of a Case; seeded by the case, so every test that
    names the same case sees the same tensors."""
    seed = (4242 + 11 * case.sq + 5 * case.sk + 3 * case.n + case.nk
            + case.d + seed_offset)
    if case.family == "seam_weighted":
        return seam_weighted(case.b, case.sq, case.sk, case.n, case.nk,
                             case.d, dtype, seed)
    assert case.family == "diag_needle" and case.causal
    return diag_needle(case.b, case.sq, case.n, case.nk, case.d, dtype, seed)


ROUND2_BETA_DROP = 2.5


def round2_kv(case, dtype):
    """(k, v) of the carry-in tests' second, unmasked round: Sk more keys
    for the same q, drawn with another seed.  They are seam_weighted keys
    (seam_vector depends on d alone, so against a seam_weighted q their
    seam keys are weighted and the second call's tail is a seam too) at
    beta = ln(sk) - ROUND2_BETA_DROP.  At the full beta they halve every
    first-round pair's share of the row, and the first round's
    tail_exclusive and last_tile_skipped mutants drop to 2.3 and 2.9 bf16
    gates; at -2.5 a second-round seam key still weighs as much as 0.08 Sk
    ordinary keys and every first-round mutant but the two listed in
    tests/test_gate_sensitivity_cpu.py stays above 3.  Against a
    diag_needle q they are ordinary keys."""
    beta = math.log(max(case.sk, 2)) - ROUND2_BETA_DROP
    _, k, v, _ = seam_weighted(case.b, case.sq, case.sk, case.n, case.nk,
                               case.d, dtype, 9001 + case.sk + case.d,
                               beta=beta)
    return k, v


# Dominated rounds: round2_kv moved along the seam direction until a causal
# carry-in round on them lies wholly below ("below") or above ("above") what
# the state carries.  A key's score moves by gain (1 + z / sqrt(d)), z ~
# N(0, 1) from q's own component along u (|z| reaches 3.5 over the rows);
# 80 leaves every second-round score of a row at least 30 from the row's
# carried max at d = 64 and 128 (tests/test_boundary_inputs_cpu.py), and at
# most 130: exp2(-130 log2 e) is 0 in fp32, the carried side must vanish.
DOMINATED_GAIN = 80.0
DOMINATED_MIN_GAP = 30.0
DOMINATED_CASES = [c for c in CASES
                   if c.family == "seam_weighted" and c.causal
                   and c.sq == 328 and (c.n, c.nk) == (4, 2)]


def dominated_kv(case, dtype, which):
    """(k, v) of a second round whose every score is DOMINATED_MIN_GAP or
    more below / above the first round's row max."""
    sign = {"below": -1.0, "above": 1.0}[which]
    k2, v2 = round2_kv(case, torch.float32)
    k2 = k2 + sign * (DOMINATED_GAIN / math.sqrt(case.d)) * seam_vector(case.d)
    return k2.to(dtype), v2.to(dtype)


def dtype_name(dtype):
    return "fp16" if dtype == torch.float16 else "bf16"


def case_id(case):
    return (f"{case.family}-{case.sq}x{case.sk}-n{case.n}k{case.nk}-"
            f"d{case.d}-{'causal' if case.causal else 'full'}")
