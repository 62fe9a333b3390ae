"""fp32 eager attention with injectable boundary errors — TEST
INFRASTRUCTURE ONLY.

Same math as ``oracle.eager_attention`` (forward) and ``oracle.tile_bwd``
(backward), restated so that the pieces a kernel predicate decides can be
swapped: an explicit ``[Sq, Sk]`` allow-mask, a weight on each (q row, key)
term of the dK/dV sums, the q-head -> kv-head map and the batch K is read
from.  ``MUTANTS`` is a named list of such swaps, each imitating one
off-by-one in a kernel predicate (cited with file and line).

``round_dtype`` rounds P (forward and dV), dS (dQ and dK) and the o that
feeds delta to the input dtype: the kernels' legitimate low-precision
rounding, emulated on the unmutated math.

tests/test_gate_sensitivity_cpu.py scores both against the parity gates:
every mutant must be rejected, the rounding emulation must pass.
"""

import dataclasses
from collections import namedtuple
from typing import Callable, Optional, Tuple

import torch

Ctx = namedtuple("Ctx", "b sq sk n nk causal")


@dataclasses.dataclass
class Spec:
    allow: torch.Tensor            # [Sq, Sk(+1 with dup_tail)] bool
    kv_weight: torch.Tensor        # [Sq, Sk(+1)] weight of a pair in dK/dV
    head_map: Tuple[int, ...]      # q head -> kv head
    k_batch: Tuple[int, ...]       # batch -> batch K is read from
    dup_tail: bool = False         # key Sk = a duplicate of row Sk-1

    def same_as(self, other):
        return (self.dup_tail == other.dup_tail
                and self.head_map == other.head_map
                and self.k_batch == other.k_batch
                and torch.equal(self.allow, other.allow)
                and torch.equal(self.kv_weight, other.kv_weight))


def base_spec(ctx):
    allow = torch.ones(ctx.sq, ctx.sk, dtype=torch.bool)
    if ctx.causal:
        assert ctx.sq == ctx.sk
        allow = allow.tril()
    g = ctx.n // ctx.nk
    return Spec(allow, torch.ones(ctx.sq, ctx.sk),
                tuple(h // g for h in range(ctx.n)), tuple(range(ctx.b)))


def _bnsd(t):
    return t.to(torch.float32).permute(0, 2, 1, 3)


def _expand(k, v, spec):
    """K/V as each q head sees them: [B, N, Sk(+1), D] fp32."""
    kf = _bnsd(k)[list(spec.k_batch)][:, list(spec.head_map)]
    vf = _bnsd(v)[:, list(spec.head_map)]
    if spec.dup_tail:
        kf = torch.cat([kf, kf[:, :, -1:]], dim=2)
        vf = torch.cat([vf, vf[:, :, -1:]], dim=2)
    return kf, vf


def _rnd(t, dtype):
    return t if dtype is None else t.to(dtype).to(torch.float32)


def forward(q, k, v, scale, spec, round_dtype=None):
    """(o [B,Sq,N,D], lse [B,N,Sq]) fp32.  With round_dtype the
    un-normalised P = exp(s - rowmax) is rounded before the PV product and
    l stays the fp32 sum, as in the kernels."""
    qf = _bnsd(q)
    kf, vf = _expand(k, v, spec)
    s = torch.matmul(qf, kf.transpose(-2, -1)) * scale
    s = s.masked_fill(~spec.allow, float("-inf"))
    m = s.amax(dim=-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(dim=-1, keepdim=True)
    o = torch.matmul(_rnd(p, round_dtype), vf) / l
    lse = (m + torch.log(l)).squeeze(-1)
    return o.permute(0, 2, 1, 3).contiguous(), lse


def backward(do, q, k, v, o, lse, scale, spec, round_dtype=None):
    """(dq [B,Sq,N,D], dk, dv [B,Sk,Nk,D]) fp32: oracle.tile_bwd's math,
        p = exp(s - lse); dv += p^T do; ds = p (do v^T - delta) scale;
        dq = ds k; dk += ds^T q,
    with delta = rowsum(o * do)."""
    qf, dof = _bnsd(q), _bnsd(do)
    kf, vf = _expand(k, v, spec)
    delta = (_rnd(_bnsd(o), round_dtype) * dof).sum(-1, keepdim=True)
    s = torch.matmul(qf, kf.transpose(-2, -1)) * scale
    s = s.masked_fill(~spec.allow, float("-inf"))
    p = torch.exp(s - lse.unsqueeze(-1))
    dp = torch.matmul(dof, vf.transpose(-2, -1))
    ds = p * (dp - delta) * scale
    p_r, ds_r = _rnd(p, round_dtype), _rnd(ds, round_dtype)
    dq = torch.matmul(ds_r, kf)
    dv_h = torch.matmul((p_r * spec.kv_weight).transpose(-2, -1), dof)
    dk_h = torch.matmul((ds_r * spec.kv_weight).transpose(-2, -1), qf)
    sk, nk = k.shape[1], k.shape[2]
    dk = torch.zeros(k.shape[0], nk, sk, k.shape[3])
    dv = torch.zeros_like(dk)
    for h, kvh in enumerate(spec.head_map):
        # a duplicated tail key has no row of its own to land in
        dk[:, kvh] += dk_h[:, h, :sk]
        dv[:, kvh] += dv_h[:, h, :sk]
    perm = lambda t: t.permute(0, 2, 1, 3).contiguous()
    return perm(dq), perm(dk), perm(dv)


def gate_ratio(out, ref, rtol, atol):
    """max |out - ref| / (atol + rtol |ref|): > 1 fails assert_close."""
    r = (out - ref).abs() / (atol + rtol * ref.abs())
    return float(torch.nan_to_num(r, nan=float("inf")).max())


# ---- the mutants ----------------------------------------------------------

@dataclasses.dataclass
class Mutant:
    name: str
    cites: str                      # the kernel predicate it imitates
    stages: Tuple[str, ...]         # "fwd": judged on o/lse; "bwd": dq/dk/dv
    apply: Callable[[Spec, Ctx], Optional[Spec]]  # None: not applicable


def _copy(spec, **kw):
    return dataclasses.replace(
        spec, allow=spec.allow.clone(), kv_weight=spec.kv_weight.clone(), **kw)


def _tail_exclusive(spec, c):
    m = _copy(spec)
    m.allow[:, c.sk - 1] = False
    return m


def _tail_inclusive(spec, c):
    if c.causal:  # key Sk lies above every row's diagonal
        return None
    m = _copy(spec, dup_tail=True)
    m.allow = torch.cat([m.allow, torch.ones(c.sq, 1, dtype=torch.bool)], 1)
    m.kv_weight = torch.cat([m.kv_weight, torch.ones(c.sq, 1)], 1)
    return m


def _strict_diag(spec, c):
    if not c.causal:
        return None
    m = _copy(spec)
    i = torch.arange(32, max(32, c.sq))
    m.allow[i, i] = False
    return m


def _superdiag_leak(spec, c):
    if not c.causal:
        return None
    m = _copy(spec)
    i = torch.arange(0, c.sq - 1)
    m.allow[i, i + 1] = True
    return m


def _full_subtile_early(spec, c):
    if not c.causal:
        return None
    m = _copy(spec)
    m.allow[256:288, 256:288] = True
    return m


def _last_tile_skipped(spec, c):
    if not c.causal:
        return None
    m = _copy(spec)
    m.allow[224:256, 192:256] = False
    return m


def _bwd_t0_late(spec, c):
    if not c.causal:
        return None
    m = _copy(spec)
    m.kv_weight[256:288, 256:] = 0.0
    return m


def _q_tail_twice(spec, c):
    m = _copy(spec)
    m.kv_weight[c.sq - 1] = 2.0
    return m


def _head_map_mod(spec, c):
    return _copy(spec, head_map=tuple(h % c.nk for h in range(c.n)))


def _batch1_reads_batch0_k(spec, c):
    if c.b < 2:
        return None
    return _copy(spec, k_batch=(0, 0) + tuple(range(2, c.b)))


MUTANTS = [
    Mutant("tail_exclusive",
           "kv_g < Sk taken as kv_g < Sk - 1: attn_fwd.hip:221 (mask_sub), "
           "attn_bwd.hip:246 (dq), :516 (dk/dv), :846 (fused)",
           ("fwd", "bwd"), _tail_exclusive),
    Mutant("tail_inclusive",
           "kv_g < Sk taken as kv_g <= Sk, admitting the clamped re-load of "
           "row Sk-1 (attn_fwd.hip:409, attn_bwd.hip:168) as key Sk",
           ("fwd", "bwd"), _tail_inclusive),
    Mutant("strict_diag_ge32",
           "kv_g <= q_row taken as kv_g < q_row for q_row >= 32: "
           "attn_fwd.hip:221, attn_bwd.hip:246, q_g >= kv_col at :516",
           ("fwd", "bwd"), _strict_diag),
    Mutant("superdiag_leak",
           "kv_g <= q_row taken as kv_g <= q_row + 1: attn_fwd.hip:221, "
           "attn_bwd.hip:246, :516",
           ("fwd", "bwd"), _superdiag_leak),
    Mutant("full_subtile_early",
           "full = ... kv0 + KVBLK - 1 <= qb taken one subtile early: "
           "attn_fwd.hip:482 leaves the 32x32 diagonal subtile at row 256 "
           "unmasked",
           ("fwd",), _full_subtile_early),
    Mutant("last_tile_skipped",
           "active = kv0 <= qb + 31 / kv_limit = (blockIdx.x + 1) * QROWS one "
           "tile short: attn_fwd.hip:476 and :174, attn_bwd.hip:201 and :156 "
           "(rows 224..255 lose keys 192..255)",
           ("fwd", "bwd"), _last_tile_skipped),
    Mutant("bwd_t0_late",
           "t0 = (blockIdx.x * 256) / QBLK one q tile late: attn_bwd.hip:388 "
           "and :741 (q rows 256..287 missing from dk/dv of keys >= 256)",
           ("bwd",), _bwd_t0_late),
    Mutant("q_tail_twice",
           "q_g < Sq dropped from the dk/dv mask: attn_bwd.hip:516 with the "
           "clamped q tail load of :408 (row Sq-1 counted twice)",
           ("bwd",), _q_tail_twice),
    Mutant("head_map_mod",
           "nkv = n / G taken as n % Nk: attn_fwd.hip:139, attn_bwd.hip:111, "
           "n0 = n * G at :352",
           ("fwd", "bwd"), _head_map_mod),
    Mutant("batch1_reads_batch0_k",
           "kp = k + b * k_sb with a zero batch stride: attn_fwd.hip:140, "
           "attn_bwd.hip:112 and :362",
           ("fwd", "bwd"), _batch1_reads_batch0_k),
]


def mutate(mutant, ctx):
    """The mutated Spec, or None where the mutant changes nothing at this
    shape (its seam is not inside it) or would leave a row without keys."""
    base = base_spec(ctx)
    spec = mutant.apply(base, ctx)
    if spec is None or spec.same_as(base):
        return None
    if not bool(spec.allow.any(dim=1).all()):
        return None
    return spec
