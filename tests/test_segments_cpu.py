"""CPU checks of the segment-id feature's parts that need no GPU:

* the masked reference of tests/segment_refs.py against the golden-pinned
  oracle run per document;
* the one-pair sensitivity of the packed inputs: moving any single
  document boundary by one token, either way, puts at least one gated
  output past its gate, for fp16's and bf16's gates;
* ``burst_attn_amd.segments`` against ``oracle.partition.get_chunk``;
* the interface's ValueErrors, raised before any ring or tile work;
* the support table and workspace layout of csrc/seg_support.h.
"""

import os
import shutil
import subprocess

import pytest
import torch

import oracle
from oracle.partition import get_chunk

from . import segment_refs as sr
from .boundary_refs import gates

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "burst_attn_amd", "csrc")


# ---- reference == oracle per document -------------------------------------

@pytest.mark.parametrize("causal", [False, True])
def test_reference_equals_oracle_per_document(causal):
    b, s, n, d = 2, sr.CAUSAL_S, 2, 64
    cu = sr.CAUSAL_CU
    ids = sr.ids_from_cu(cu, s).expand(b, -1).contiguous()
    g = torch.Generator().manual_seed(99)
    q, k, v, do = (torch.randn(b, s, n, d, generator=g) for _ in range(4))
    sc = 1.0 / d ** 0.5
    o, lse = sr.seg_fwd(q, k, v, sc, causal, ids, ids)
    dq, dk, dv = sr.seg_bwd(do, q, k, v, lse, sc, causal, ids, ids, o=o)
    for a, e in zip(cu[:-1], cu[1:]):
        sl = slice(a, e)
        o_d, lse_d = oracle.tile_fwd(q[:, sl], k[:, sl], v[:, sl], sc, causal)
        dq_d, dk_d, dv_d = oracle.tile_bwd(do[:, sl], q[:, sl], k[:, sl],
                                           v[:, sl], lse_d, sc, causal, o=o_d)
        for got, want in ((o[:, sl], o_d), (lse[:, :, sl], lse_d),
                          (dq[:, sl], dq_d), (dk[:, sl], dk_d),
                          (dv[:, sl], dv_d)):
            torch.testing.assert_close(got, want, rtol=2e-5, atol=2e-5)


def test_reference_never_visible_rows():
    c = sr.rect_case(2, 2, 64, torch.float16)
    dead = c["q_seg"][0] == 9
    assert dead.sum() == 6
    assert (c["o"][:, dead] == 0).all() and c["lse"][:, :, dead].isinf().all()
    assert (c["dq"][:, dead] == 0).all()
    unseen = (c["kv_seg"][0] == 5) | (c["kv_seg"][0] == 6)
    assert (c["dk"][:, unseen] == 0).all() and (c["dv"][:, unseen] == 0).all()
    for name in ("o", "dq", "dk", "dv"):
        assert c[name].isfinite().all(), name


# ---- one-pair sensitivity ---------------------------------------------------

def _moved(cu, i, step):
    out = list(cu)
    out[i] += step
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("d,n,nk", [(64, 2, 2), (128, 4, 2)])
def test_moving_one_boundary_is_caught(dtype, d, n, nk):
    """The reference under ids whose boundary i sits one token off must miss
    a gate of the reference under the true ids: what a kernel that puts one
    token in the wrong document would produce."""
    c = sr.causal_case(n, nk, d, dtype)
    gt = gates(dtype, n // nk)
    cu = list(sr.CAUSAL_CU)
    for i in range(1, len(cu) - 1):
        for step in (-1, 1):
            wrong_cu = _moved(cu, i, step)
            if not all(a <= b for a, b in zip(wrong_cu[:-1], wrong_cu[1:])):
                continue
            ids = sr.ids_from_cu(wrong_cu, sr.CAUSAL_S).expand(2, -1)
            o, lse = sr.seg_fwd(c["q"], c["k"], c["v"], c["scale"], True, ids,
                                ids)
            dq, dk, dv = sr.seg_bwd(c["do"], c["q"], c["k"], c["v"], lse,
                                    c["scale"], True, ids, ids, o=o)
            worst = {nm: sr.exceeds(t, c[nm], gt[nm]) for nm, t in
                     (("o", o), ("lse", lse), ("dq", dq), ("dk", dk),
                      ("dv", dv))}
            assert max(worst.values()) > 1.0, (cu[i], step, worst)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_low_precision_rounding_passes_the_gates(dtype):
    """The gates still admit what a correct low-precision kernel does: P
    rounded to the input dtype before the PV product."""
    c = sr.causal_case(4, 2, 128, dtype)
    gt = gates(dtype, 2)
    from .gqa_cpu_provider import expand_kv
    q = c["q"].float().transpose(1, 2)
    k = expand_kv(c["k"], 4).float().transpose(1, 2)
    v = expand_kv(c["v"], 4).float().transpose(1, 2)
    m = sr.mask_of(c["q_seg"], c["kv_seg"], True)[:, None]
    s = (q @ k.transpose(-1, -2) * c["scale"]).masked_fill(~m, float("-inf"))
    mx = s.amax(-1, keepdim=True)
    p = torch.exp(s - mx)
    o = (p.to(dtype).float() @ v) / p.sum(-1, keepdim=True)
    assert sr.exceeds(o.transpose(1, 2), c["o"], gt["o"]) <= 1.0


# ---- the one-GPU ring replay's helper, on the oracle provider ----------------

@pytest.mark.parametrize("layout", ["zigzag", "striped"])
def test_segment_replay_helper_on_cpu(layout):
    """tests/segment_ring_rounds.replay_ring_seg composes the product's
    tile_window tiles and the chunked ids to the full-sequence reference."""
    from . import segment_ring_rounds as srr
    from .segment_cpu_provider import SegOracleTileProvider

    c = srr.ring_case(3, 64, torch.float32)
    got = srr.replay_ring_seg(SegOracleTileProvider(), c["q"], c["k"], c["v"],
                              c["do"], c["q_seg"], 3, c["scale"], True, layout)
    for name, out in zip(("o", "lse", "dq", "dk", "dv"), got):
        torch.testing.assert_close(out, c[name], rtol=1e-4, atol=1e-4,
                                   msg=lambda m, name=name: f"{name}: {m}")


# ---- segments.py ------------------------------------------------------------

def test_ids_from_cu_seqlens():
    from burst_attn_amd import segment_ids_from_cu_seqlens

    ids = segment_ids_from_cu_seqlens([0, 1, 4, 4, 6], 8)
    assert ids.dtype == torch.int32
    assert ids.tolist() == [0, 1, 1, 1, 3, 3, 4, 4]  # empty doc 2, pad = 4
    assert torch.equal(segment_ids_from_cu_seqlens(sr.CAUSAL_CU, sr.CAUSAL_S),
                       sr.ids_from_cu(sr.CAUSAL_CU, sr.CAUSAL_S))
    for bad in ([1, 4], [0, 5, 3], [0, 9]):
        with pytest.raises(ValueError):
            segment_ids_from_cu_seqlens(bad, 8)


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_local_ids_match_partition(world):
    from burst_attn_amd import local_segment_ids

    s = 24 * world
    ids = torch.arange(2 * s, dtype=torch.int32).reshape(2, s)
    for rank in range(world):
        for layout, kw in (("contiguous", {}), ("zigzag", {"zigzag": True}),
                           ("striped", {"striped": True})):
            got = local_segment_ids(ids, layout, rank, world)
            assert torch.equal(got, get_chunk(ids, 1, rank, world, **kw))
            # local order is globally increasing in every layout
            assert (got[:, 1:] > got[:, :-1]).all()
    with pytest.raises(ValueError):
        local_segment_ids(ids, "ring", 0, world)
    with pytest.raises(ValueError):
        local_segment_ids(ids, "striped", world, world)


# ---- interface validation ---------------------------------------------------

@pytest.mark.parametrize("striped", [False, True])
def test_bad_segment_ids_raise_before_any_work(striped):
    """No process group and no provider exist here: the checks come first."""
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    func = burst_attn_func_striped if striped else burst_attn_func
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(2, 32, 2, 64, generator=g) for _ in range(3))
    good = torch.zeros(2, 32, dtype=torch.int32)
    for bad, pat in ((good[:, :31], r"\[B, S_local\]"),
                     (good[:1], r"\[B, S_local\]"),
                     (good.float(), "int32 or int64"),
                     (good.to(torch.int16), "int32 or int64"),
                     (good.tolist(), "tensor"),
                     (good.to("meta"), "is on")):
        with pytest.raises(ValueError, match=pat):
            func(q, k, v, None, "cuda", True, segment_ids=bad)


# ---- seg_support.h ------------------------------------------------------------

MAIN = r"""
#include <stdio.h>
#include "seg_support.h"
int main() {
  char which;
  int a, b, c, d, e;
  while (scanf(" %c %d %d %d %d %d", &which, &a, &b, &c, &d, &e) == 6) {
    ba_seg_verdict v{};
    if (which == 'f') {
      ba_fwd_knobs k;
      k.vpath = a; k.subt = b; k.nt = c; k.nbuf = d; k.kreg = e;
      v = ba_seg_fwd_support(k);
    } else if (which == 'b') {
      ba_bwd_knobs k;
      k.fused = a; k.dk_flip = b; k.dq_pipe = c; k.dkq_dbg = d;
      v = ba_seg_bwd_support(k);
    } else {
      const ba_seg_ws_layout w = ba_seg_ws(a, b, c);
      printf("%lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)w.flags_kv,
             (long long)w.flags_q, (long long)w.kv_tile_mm,
             (long long)w.q_blk_range, (long long)w.q_tile_mm,
             (long long)w.kv_blk_range, (long long)w.words,
             (long long)ba_seg_ws_bytes(a, b, c));
      continue;
    }
    if (v.knob) printf("no %s %d\n", v.knob, v.value); else printf("ok\n");
  }
  return 0;
}
"""

SUPPORT = [
    ("f 0 1 512 2 0", "ok"),                    # the defaults
    ("f 1 1 512 2 0", "no BA_FWD_VPATH 1"),
    ("f 0 0 512 2 0", "no BA_FWD_SUBT 0"),
    ("f 0 2 512 2 0", "no BA_FWD_SUBT 2"),
    ("f 0 3 512 2 0", "no BA_FWD_SUBT 3"),
    ("f 0 1 256 2 0", "no BA_FWD_NT 256"),
    ("f 0 1 512 4 0", "no BA_FWD_NBUF 4"),
    ("f 0 1 512 2 1", "no BA_FWD_KREG 1"),
    ("f 1 1 256 4 2", "no BA_FWD_KREG 2"),      # the pinning knob is named
    ("f 0 7 512 2 0", "ok"),                    # a bad value is select's to report
    ("b 0 0 0 0 0", "ok"),
    ("b 0 0 0 2 0", "ok"),                      # DKQ_DBG is unused outside atomic6
    ("b 1 0 0 0 0", "no BA_BWD_FUSED 1"),
    ("b 2 0 0 0 0", "no BA_BWD_FUSED 2"),
    ("b 0 1 0 0 0", "no BA_BWD_DK_FLIP 1"),
    ("b 0 0 1 0 0", "no BA_DQ_PIPE 1"),
    # B=2, Sq=328, Sk=96: 6/2 q tiles/blocks, 2/1 kv tiles/blocks
    ("w 2 328 96 0 0", "0 2 4 12 20 44 48 192"),
]


@pytest.fixture(scope="module")
def support(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if shutil.which("c++"):
        cc = ["c++"]
    elif shutil.which(hipcc):
        cc = [hipcc, "-x", "c++"]
    else:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("seg_support")
    src, exe = d / "main.cpp", d / "main"
    src.write_text(MAIN)
    subprocess.run(cc + ["-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                         str(src), "-o", str(exe)], check=True)
    stdin = "".join(line + "\n" for line, _ in SUPPORT)
    return subprocess.run([str(exe)], input=stdin, capture_output=True,
                          text=True, check=True).stdout.splitlines()


@pytest.mark.parametrize("i", range(len(SUPPORT)),
                         ids=[s.replace(" ", "-") for s, _ in SUPPORT])
def test_support_table(support, i):
    assert support[i] == SUPPORT[i][1], SUPPORT[i][0]
