"""CPU check of the V^T image layout (burst_attn_amd/csrc/vt_image.h).

The header is host-only, so a plain C++ compiler builds it with a small
main that prints the element offset of V[b, kv, nkv, d] for a list of
points and the tile count, byte size and workspace check for a list of
shapes.  The expected values are the same layout computed in numpy: V
zero-padded to a multiple of 64 rows, reshaped to [B, T, 64, Nk, D] and
permuted to [B, Nk, T, D, 64].
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "burst_attn_amd", "csrc")

MAIN = r"""
#include <stdio.h>
#include "vt_image.h"
// stdin lines: "o B Nk Sk D b nkv kv d" -> element offset;
//              "s B Nk Sk D ws"         -> tiles, bytes, ws fits;
//              "r Sq G"                 -> reuse, auto rule takes the image
int main() {
  char op;
  while (scanf(" %c", &op) == 1) {
    long long B, Nk, Sk, D, b, nkv, kv, d, ws, Sq, G;
    if (op == 'o') {
      if (scanf("%lld %lld %lld %lld %lld %lld %lld %lld", &B, &Nk, &Sk, &D,
                &b, &nkv, &kv, &d) != 8) return 1;
      printf("%lld\n", (long long)ba_vt_offset(Nk, Sk, D, b, nkv, kv, d));
    } else if (op == 's') {
      if (scanf("%lld %lld %lld %lld %lld", &B, &Nk, &Sk, &D, &ws) != 5)
        return 1;
      printf("%lld %lld %d\n", (long long)ba_vt_tiles(Sk),
             (long long)ba_vt_bytes(B, Nk, Sk, D),
             (int)ba_vt_workspace_fits(ws, B, Nk, Sk, D));
    } else if (op == 'r') {
      if (scanf("%lld %lld", &Sq, &G) != 2) return 1;
      printf("%lld %d\n", (long long)ba_vt_reuse(Sq, G),
             (int)(ba_vt_reuse(Sq, G) >= BA_VT_AUTO_MIN_REUSE));
    } else {
      return 1;
    }
  }
  printf("threshold %lld\n", (long long)BA_VT_AUTO_MIN_REUSE);
  return 0;
}
"""

# (B, Nk, Sk, D)
SHAPES = [(2, 2, 1, 64), (2, 2, 63, 128), (1, 3, 64, 64), (2, 2, 65, 128),
          (2, 2, 296, 64), (1, 1, 128, 128), (1, 32, 262144, 128),
          (3, 8, 1 << 22, 128)]
REUSE = [(1, 1), (256, 1), (257, 1), (1024, 1), (256, 4), (2048, 1),
         (262144, 1), (300, 8)]


def _points(B, Nk, Sk, D):
    """corners, the tile boundaries and a few interior points"""
    kvs = sorted({0, Sk - 1, min(63, Sk - 1), min(64, Sk - 1), Sk // 2,
                  (Sk - 1) // 64 * 64})
    return [(b, n, kv, d) for b in {0, B - 1} for n in {0, Nk - 1}
            for kv in kvs for d in {0, 1, D // 2 + 3, D - 1}]


def _numpy_offsets(B, Nk, Sk, D):
    """element offset in the image of every V[b, kv, nkv, d], by the
    docstring's pad / reshape / permute on an array of source indices"""
    T = (Sk + 63) // 64
    src = np.full((B, T * 64, Nk, D), -1, dtype=np.int64)
    src[:, :Sk] = np.arange(B * Sk * Nk * D).reshape(B, Sk, Nk, D)
    img = src.reshape(B, T, 64, Nk, D).transpose(0, 3, 1, 4, 2).reshape(-1)
    where = np.full(B * Sk * Nk * D, -1, dtype=np.int64)
    valid = img >= 0
    where[img[valid]] = np.nonzero(valid)[0]
    return where.reshape(B, Sk, Nk, D), img.size


def _lines():
    lines = []
    for B, Nk, Sk, D in SHAPES:
        size = B * Nk * ((Sk + 63) // 64) * D * 64 * 2
        for ws in (size, size - 1, 0, size + 16):
            lines.append(("s", B, Nk, Sk, D, ws))
    for B, Nk, Sk, D in SHAPES[:6]:
        for p in _points(B, Nk, Sk, D):
            lines.append(("o", B, Nk, Sk, D) + p)
    for sq, g in REUSE:
        lines.append(("r", sq, g))
    return lines


def _compile(tmp, extra=()):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if shutil.which("c++"):
        cc = ["c++"]
    elif shutil.which(hipcc):
        cc = [hipcc, "-x", "c++"]
    else:
        pytest.skip("no host C++ compiler")
    src, exe = tmp / "main.cpp", tmp / "main"
    src.write_text(MAIN)
    subprocess.run(cc + ["-std=c++17", "-Wall", "-Werror", *extra, "-I", CSRC,
                         str(src), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = _compile(tmp_path_factory.mktemp("vt_image"))
    lines = _lines()
    stdin = "".join(" ".join(map(str, ln)) + "\n" for ln in lines)
    out = subprocess.run([str(exe)], input=stdin, capture_output=True,
                         text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines) + 1
    return dict(zip(lines, out)), out[-1]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_size_and_workspace_check(printed, shape):
    B, Nk, Sk, D = shape
    T = (Sk + 63) // 64
    size = B * Nk * T * D * 64 * 2
    got = printed[0]
    assert got[("s", B, Nk, Sk, D, size)] == f"{T} {size} 1"
    assert got[("s", B, Nk, Sk, D, size + 16)] == f"{T} {size} 1"
    # one byte short, or nothing: the launcher must refuse
    assert got[("s", B, Nk, Sk, D, size - 1)] == f"{T} {size} 0"
    assert got[("s", B, Nk, Sk, D, 0)] == f"{T} {size} 0"


@pytest.mark.parametrize("shape", SHAPES[:6],
                         ids=lambda s: "x".join(map(str, s)))
def test_offsets_match_numpy_permutation(printed, shape):
    B, Nk, Sk, D = shape
    where, n_img = _numpy_offsets(B, Nk, Sk, D)
    assert n_img * 2 == int(printed[0][("s", B, Nk, Sk, D, 0)].split()[1])
    for b, n, kv, d in _points(B, Nk, Sk, D):
        got = int(printed[0][("o", B, Nk, Sk, D, b, n, kv, d)])
        assert got == where[b, kv, n, d], (b, n, kv, d)


def test_auto_rule(printed):
    got, last = printed
    thr = int(last.split()[1])
    assert thr >= 1
    for sq, g in REUSE:
        reuse = (sq + 255) // 256 * g
        assert got[("r", sq, g)] == f"{reuse} {int(reuse >= thr)}"
