"""Block-sparse attention without a GPU: the interface's refusals, the ring on
gloo with an oracle tile provider that applies ``blocks`` by expanding it, and
csrc/blk_support.h compiled by the host C++17 compiler.
"""

import os
import shutil
import subprocess

import pytest
import torch

from oracle.partition import get_chunk

from .gloo_ranks import run_ranks
from .test_ring_cpu import ATOL, RTOL
from . import segment_refs as sr
from .window_cpu_provider import WindowOracleTileProvider, merge_with_inf

BS, S_LOCAL, B, N, NK, D = 64, 128, 2, 4, 2, 16
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                    "burst_attn_amd", "csrc")


def _elements(m, bs):
    return m.bool().repeat_interleave(bs, 2).repeat_interleave(bs, 3)


class BlockOracleTileProvider(WindowOracleTileProvider):
    """``blocks=(mask2d, BS)`` (one mask head) expanded to an element mask,
    ANDed with the causal triangle, for the dense masked reference; what it
    was handed is recorded."""

    def __init__(self):
        super().__init__()
        self.fwd_blocks, self.bwd_blocks = [], []

    @staticmethod
    def _emask(q, k, causal, blocks):
        m, bs = blocks
        assert m.dtype == torch.uint8 and m.shape[1:] == (
            1, q.shape[1] // bs, k.shape[1] // bs)
        e = _elements(m, bs)[:, 0].expand(q.shape[0], -1, -1)
        return e & torch.ones(e.shape[1:], dtype=torch.bool).tril() \
            if causal else e

    def fwd_accum(self, state, q, k, v, scale, causal, row_offset=0,
                  blocks=None):
        self.fwd_blocks.append((blocks[0].clone(), causal, row_offset))
        o_i, lse_i = sr.seg_fwd(q, k, v, scale, False, None, None,
                                mask=self._emask(q, k, causal, blocks))
        o, lse = state
        sl = slice(row_offset, row_offset + q.shape[1])
        o[:, sl], lse[:, sl] = merge_with_inf(o[:, sl], lse[:, sl], o_i, lse_i)
        return state

    def bwd_accum(self, do, q, k, v, delta, lse, scale, causal, deterministic,
                  dq, dk, dv, blocks=None):
        self.bwd_blocks.append((blocks[0].clone(), causal))
        grads = sr.seg_bwd(do, q, k, v, lse, scale, False, None, None,
                           delta=delta, mask=self._emask(q, k, causal, blocks))
        for acc, g in zip((dq, dk, dv), grads):
            acc += g


def _worker(rank, world, causal, opt_bwd):
    from burst_attn_amd import burst_attn_func
    from burst_attn_amd.interface import (_block_view, block_tiles,
                                          get_partition_id)
    from burst_attn_amd.tile import _set_tile_provider_for_testing

    P = BlockOracleTileProvider()
    _set_tile_provider_for_testing(P)
    s = S_LOCAL * world
    g = torch.Generator().manual_seed(99 + world)
    q = torch.randn(B, s, N, D, generator=g)
    k = torch.randn(B, s, NK, D, generator=g)
    v = torch.randn(B, s, NK, D, generator=g)
    do = torch.randn(B, s, N, D, generator=g)
    M = (torch.rand(1, 1, s // BS, s // BS, generator=g) < 0.5)
    M[..., 1, :] = False  # a dead query block
    M[..., :, 2] = False  # a key block nobody sees
    e = _elements(M, BS)[:, 0].expand(B, s, s)
    if causal:
        e = e & torch.ones(s, s, dtype=torch.bool).tril()
    sc = 1.0 / D ** 0.5
    o_ref, lse_ref = sr.seg_fwd(q, k, v, sc, False, None, None, mask=e)
    ref = (o_ref, *sr.seg_bwd(do, q, k, v, lse_ref, sc, False, None, None,
                              o=o_ref, mask=e))
    ch = lambda t: get_chunk(t, 1, rank, world, zigzag=causal, striped=False)
    slab = lambda r: get_chunk(M, 2, r, world, zigzag=causal, striped=False)
    qc, kc, vc = (ch(t).requires_grad_() for t in (q, k, v))
    o = burst_attn_func(qc, kc, vc, None, "cuda", causal, opt_bwd,
                        block_mask=slab(rank), block_size=BS)
    got = (o, *torch.autograd.grad(o, (qc, kc, vc), ch(do)))
    for nm, out, want in zip(("o", "dq", "dk", "dv"), got, ref):
        torch.testing.assert_close(out, ch(want), rtol=RTOL, atol=ATOL,
                                   msg=lambda t, nm=nm: f"{nm}: {t}")

    # what the provider was handed: in the forward views of this rank's slab,
    # in the backward views of the slab of the round's q rank (it travelled
    # with q), on this rank's own key-block columns
    want_f, want_b = [], []
    for r in range(1, world + 1):
        src = get_partition_id([None, None], r, None)
        for qw, kw, kv0, tc in block_tiles(rank, src, world, S_LOCAL, causal):
            sub = _block_view(slab(rank).to(torch.uint8), BS, qw, kw, kv0)
            if sub.any():
                want_f.append((sub, tc, qw.start))
        for qw, kw, kv0, tc in block_tiles(src, rank, world, S_LOCAL, causal):
            want_b.append((_block_view(slab(src).to(torch.uint8), BS, qw, kw,
                                       kv0), tc))
    assert P.empty_states == 1
    for got, want in ((P.fwd_blocks, want_f), (P.bwd_blocks, want_b)):
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a[0].shape == b[0].shape and torch.equal(a[0], b[0])
            assert a[1:] == b[1:]


@pytest.mark.parametrize("opt_bwd", [False, True])
@pytest.mark.parametrize("causal", [True, False])
def test_block_mask_ring_matches_masked_attention(causal, opt_bwd):
    run_ranks(_worker, 2, causal, opt_bwd, what="block-sparse ring")


# the interface's refusals need no process group
def _refusal_cases():
    q = torch.randn(1, 256, 2, 16)
    m = torch.ones(1, 1, 4, 4, dtype=torch.bool)
    ids = torch.zeros(1, 256, dtype=torch.int32)
    kw = lambda **k: {"block_mask": m, "block_size": 64, **k}
    return q, {
        "ids": (kw(segment_ids=ids), "block_mask.*segment_ids"),
        "window": (kw(window_size=(8, 0)), "block_mask.*window_size"),
        "softcap": (kw(softcap=30.0), "block_mask.*softcap"),
        "bs48": (kw(block_size=48), "block_size.*power of two"),
        "dtype": (kw(block_mask=m.float()), "block_mask.*bool or uint8"),
        "rows": (kw(block_mask=m[:, :, :3]), r"block_mask must be \[1 or B"),
        "cols": (kw(block_mask=m[..., :3]), r"block_mask must be \[1 or B"),
        "Hm": (kw(block_mask=m.expand(1, 3, 4, 4)),
               r"block_mask must be \[1 or B"),
        "s_local": (kw(block_size=512), "block_mask.*multiple of"),
        "device": (kw(block_mask=m.to("meta")), "block_mask is on meta"),
        "d256": ({**kw(), "q": torch.randn(1, 256, 2, 256)},
                 "head_dim 256.*block_mask"),
        "causal": ({**kw(block_mask=m[:, :, :3]), "q": q[:, :192],
                    "causal": True}, r"2 \* block_size.*zigzag"),
        "striped": ({**kw(), "striped": True}, "striped.*block_mask"),
    }


@pytest.mark.parametrize("name", sorted(_refusal_cases()[1]))
def test_interface_refusals(name):
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    q, cases = _refusal_cases()
    kw, match = cases[name]
    q, causal = kw.pop("q", q), kw.pop("causal", False)
    func = burst_attn_func_striped if kw.pop("striped", 0) else burst_attn_func
    with pytest.raises(ValueError, match=match):
        func(q, q, q, None, "cuda", causal, **kw)


# blk_support.h with the host compiler
MAIN = r"""
#include <stdio.h>
#include <vector>
#include "blk_support.h"

// the `holes` case of the GPU tests: Sq = 328, Sk = 392, BS = 64, every other
// key block set; prints the workspace size, then every list of both sides
int main() {
  const int Sq = 328, Sk = 392, nq = 6, nk = 7;
  std::vector<uint8_t> m(nq * nk, 0);
  for (int r = 0; r < nq; ++r)
    for (int c = 0; c < nk; c += 2) m[r * nk + c] = 1;
  printf("%lld %lld\n", (long long)ba_blk_ws_bytes(1, 1, Sq, Sk),
         (long long)ba_blk_ws_bytes(2, 3, Sq, Sk));
  std::vector<uint32_t> out(16);
  for (int side = 0; side < 2; ++side) {
    const ba_blk_plane p = {m.data(), side ? 1 : nk, side ? nk : 1, 6};
    const int S_own = side ? Sk : Sq, S_str = side ? Sq : Sk;
    for (int blk = 0; blk < ba_blk_blocks(S_own); ++blk) {
      const int n = (int)ba_blk_build_list(p, blk, S_own, S_str, false,
                                           side == 0, out.data());
      printf("%d %d:", side, blk);
      for (int i = 0; i < n; ++i)
        printf(" %u/%02x", out[i] & BA_BLK_TILE_MASK,
               out[i] >> BA_BLK_TILE_BITS);
      printf("\n");
    }
  }
  // causal, all set, Sq = Sk = 328: block 1, waves at rows 256, 288 and 320
  std::vector<uint8_t> ones(36, 1);
  const ba_blk_plane p = {ones.data(), 6, 1, 6};
  const int n = (int)ba_blk_build_list(p, 1, 328, 328, true, true, out.data());
  printf("c:");
  for (int i = 0; i < n; ++i)
    printf(" %u/%02x", out[i] & BA_BLK_TILE_MASK, out[i] >> BA_BLK_TILE_BITS);
  printf("\n");
  return 0;
}
"""


def test_blk_support_header(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "main.cpp").write_text(MAIN)
    exe = tmp_path / "blk_support_test"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                    str(tmp_path / "main.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True,
                         text=True).stdout.splitlines()
    # words = L * (nb(Sq) (1 + nt(Sk)) + nb(Sk) (1 + nt(Sq))), nb = ceil(S/256),
    # nt = ceil(S/64): 2 * 8 + 2 * 7 = 30 words for one list set
    assert out[0] == f"{30 * 4} {6 * 30 * 4}"
    # q-owning: key tiles 0, 2, 4, 6 (every other 64-key block); own block 0
    # has all eight waves, block 1 rows 256..327 = waves 0, 1, 2
    assert out[1] == "0 0: 0/ff 2/ff 4/ff 6/ff"
    assert out[2] == "0 1: 0/07 2/07 4/07 6/07"
    # kv-owning: own block 0 holds key blocks 0..3, of which 0 and 2 are set
    # (waves 0, 1 and 4, 5), for every q tile; block 1 key blocks 4 and 6
    # (waves 0, 1 and 4: keys 384..391 are one wave)
    assert out[3] == "1 0:" + "".join(f" {t}/33" for t in range(6))
    assert out[4] == "1 1:" + "".join(f" {t}/13" for t in range(6))
    # causal: wave 0 (rows 256..) sees tiles 0..4, so do waves 1 (288..) and
    # 2 (320..); tile 5 (keys 320..) only wave 2
    assert out[5] == "c: 0/07 1/07 2/07 3/07 4/07 5/04"
