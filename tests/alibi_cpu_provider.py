"""ALiBi reference and fp64 tile provider — TEST INFRASTRUCTURE ONLY: plain
attention with the one line ``s -= slope[b, h] * |stride * (i - j) + offset|``,
and the provider's ``alibi=`` keyword on top of it, so that the product's ring
runs on CPU (gloo).  The state is (o, lse [B,S,N,1]) in fp64."""

import math

import torch


def std_slopes(b, n):
    """[b, n]: batch row i is (1 + i) x the geometric 2 ** -(8 (h + 1) / n)."""
    h = torch.arange(1, n + 1, dtype=torch.float32)
    return torch.stack([2.0 ** (-8.0 * h / n) * (1 + i) for i in range(b)])


def alibi_scores(q, k, scale, causal, slopes=None, offset=0, stride=1):
    """Biased, masked scores [B,N,Sq,Sk] of q [B,Sq,N,D] and k [B,Sk,Nk,D]."""
    n, nk = q.shape[2], k.shape[2]
    s = torch.einsum("bqnd,bknd->bnqk", q,
                     k.repeat_interleave(n // nk, dim=2)) * scale
    i = torch.arange(q.shape[1])[:, None]
    j = torch.arange(k.shape[1])[None, :]
    if slopes is not None:
        sl = slopes.double().reshape(-1, n)[:, :, None, None]
        s = s - sl * (stride * (i - j) + offset).abs()
    return s.masked_fill(j > i, -math.inf) if causal else s


def alibi_attention(q, k, v, scale, causal, slopes=None, offset=0, stride=1):
    """(o [B,Sq,N,D], lse [B,N,Sq]) in the dtype of q (fp64 in the tests)."""
    s = alibi_scores(q, k, scale, causal, slopes, offset, stride)
    ve = v.repeat_interleave(q.shape[2] // v.shape[2], dim=2)
    return (torch.einsum("bnqk,bknd->bqnd", torch.softmax(s, -1), ve),
            torch.logsumexp(s, -1))


class AlibiTileProvider:
    def fwd_empty_state(self, q):
        b, s, n, d = q.shape
        return [torch.zeros(b, s, n, d, dtype=torch.float64),
                torch.full((b, s, n, 1), -math.inf, dtype=torch.float64)]

    def fwd_accum(self, state, q, k, v, scale, causal, row_offset=0,
                  alibi=None):
        o, lse = state = state or self.fwd_empty_state(q)
        o_i, lse_i = alibi_attention(q.double(), k.double(), v.double(), scale,
                                     causal, *(alibi or ()))
        sl = slice(row_offset, row_offset + q.shape[1])
        lse_i = lse_i.transpose(1, 2).unsqueeze(-1)
        new = torch.logaddexp(lse[:, sl], lse_i)
        o[:, sl] = (torch.exp(lse[:, sl] - new) * o[:, sl]
                    + torch.exp(lse_i - new) * o_i)
        lse[:, sl] = new
        return state

    def fwd_finalize(self, state, out_dtype):
        o, lse = state
        return (o.to(out_dtype),
                lse.squeeze(-1).transpose(1, 2).float().contiguous())

    def bwd_preprocess(self, o, do, out=None):
        delta = (o.double() * do.double()).sum(-1).transpose(1, 2).float()
        return delta.contiguous() if out is None else out.copy_(delta)

    def bwd_accum(self, do, q, k, v, delta, lse, scale, causal, deterministic,
                  dq, dk, dv, alibi=None):
        """The tile's share under the ring's merged lse and delta."""
        g = q.shape[2] // k.shape[2]
        q, k, v, do = (t.double() for t in (q, k, v, do))
        s = alibi_scores(q, k, scale, causal, *(alibi or ()))
        p = torch.exp(s - lse.double()[..., None])
        dp = torch.einsum("bqnd,bknd->bnqk", do, v.repeat_interleave(g, dim=2))
        ds = p * (dp - delta.double()[..., None]) * scale
        red = lambda t: t.reshape(*t.shape[:2], -1, g, t.shape[-1]).sum(3)
        dq += torch.einsum("bnqk,bknd->bqnd", ds, k.repeat_interleave(g, dim=2))
        dk += red(torch.einsum("bnqk,bqnd->bknd", ds, q))
        dv += red(torch.einsum("bnqk,bqnd->bknd", p, do))
