"""CPU check of the forward variant table (burst_attn_amd/csrc/fwd_variants.h).

The header is host-only, so a plain C++ compiler builds it with a small
main that prints what ba_fwd_select chooses for a list of knob tuples.
The expected values below are transcribed from the decision ladder the
table replaced (first match wins):

    KREG=1 -> <0,1,512,2,1>      KREG=2 -> <0,1,512,4,2>
    SUBT=3 -> <0,3,256,4,0>      SUBT=2 -> <0,2,512,4,0>
    NBUF=4 and NT=512 -> <VPATH,1,512,4,0>
    NT=256 -> <VPATH,1,256,2,0>
    otherwise <VPATH,SUBT,512,2,0>
"""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "burst_attn_amd", "csrc")

MAIN = r"""
#include <stdio.h>
#include "fwd_variants.h"
// stdin: one "vpath subt nt nbuf kreg" tuple per line; stdout: the variant
// ba_fwd_select picks, or the rejected knob.  First line: the variant list.
int main() {
#define PRINT_VARIANT(VP, ST, NT, NB, KR) printf("%d,%d,%d,%d,%d ", VP, ST, NT, NB, KR);
  BA_FWD_VARIANTS(PRINT_VARIANT)
  printf("\n");
  ba_fwd_knobs k;
  printf("%d,%d,%d,%d,%d\n", k.vpath, k.subt, k.nt, k.nbuf, k.kreg);
  while (scanf("%d %d %d %d %d", &k.vpath, &k.subt, &k.nt, &k.nbuf,
               &k.kreg) == 5) {
    const ba_fwd_choice c = ba_fwd_select(k);
    if (c.bad_knob)
      printf("reject %s %d\n", c.bad_knob, c.bad_value);
    else
      printf("%d,%d,%d,%d,%d\n", c.variant.vpath, c.variant.subt,
             c.variant.nt, c.variant.nbuf, c.variant.kreg);
  }
  return 0;
}
"""

# (vpath, subt, nt, nbuf, kreg) -> variant, or ("reject", knob, value)
CASES = [
    # every row of the table
    ((0, 1, 512, 2, 1), (0, 1, 512, 2, 1)),
    ((0, 1, 512, 2, 2), (0, 1, 512, 4, 2)),
    ((0, 3, 512, 2, 0), (0, 3, 256, 4, 0)),
    ((0, 2, 512, 4, 0), (0, 2, 512, 4, 0)),
    ((0, 1, 512, 4, 0), (0, 1, 512, 4, 0)),
    ((1, 1, 512, 4, 0), (1, 1, 512, 4, 0)),
    ((0, 1, 256, 2, 0), (0, 1, 256, 2, 0)),
    ((1, 1, 256, 2, 0), (1, 1, 256, 2, 0)),
    ((0, 0, 512, 2, 0), (0, 0, 512, 2, 0)),
    ((0, 1, 512, 2, 0), (0, 1, 512, 2, 0)),  # the defaults
    ((1, 0, 512, 2, 0), (1, 0, 512, 2, 0)),
    ((1, 1, 512, 2, 0), (1, 1, 512, 2, 0)),
    # precedence collisions
    ((0, 3, 512, 2, 1), (0, 1, 512, 2, 1)),  # KREG=1 beats SUBT=3
    ((1, 2, 256, 4, 2), (0, 1, 512, 4, 2)),  # KREG=2 pins the rest
    ((0, 2, 512, 2, 0), (0, 2, 512, 4, 0)),  # SUBT=2 forces NBUF=4
    ((1, 3, 512, 4, 0), (0, 3, 256, 4, 0)),  # SUBT=3 ignores VPATH/NT
    ((0, 0, 512, 4, 0), (0, 1, 512, 4, 0)),  # SUBT=0 with NBUF=4 runs SUBT=1
    ((1, 0, 256, 2, 0), (1, 1, 256, 2, 0)),  # SUBT=0 with NT=256 runs SUBT=1
    ((0, 1, 256, 4, 0), (0, 1, 256, 2, 0)),  # NT=256 with NBUF=4 runs NBUF=2
    # one rejected value per knob
    ((2, 1, 512, 2, 0), ("reject", "BA_FWD_VPATH", 2)),
    ((0, 5, 512, 2, 0), ("reject", "BA_FWD_SUBT", 5)),
    ((0, 1, 128, 2, 0), ("reject", "BA_FWD_NT", 128)),
    ((0, 1, 512, 3, 0), ("reject", "BA_FWD_NBUF", 3)),
    ((0, 1, 512, 2, 3), ("reject", "BA_FWD_KREG", 3)),
    ((0, -1, 512, 2, 0), ("reject", "BA_FWD_SUBT", -1)),
]


@pytest.fixture(scope="module")
def selected(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if shutil.which("c++"):
        cc = ["c++"]
    elif shutil.which(hipcc):
        cc = [hipcc, "-x", "c++"]
    else:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("fwd_variants")
    src, exe = d / "main.cpp", d / "main"
    src.write_text(MAIN)
    subprocess.run(cc + ["-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                         str(src), "-o", str(exe)], check=True)
    stdin = "".join(" ".join(map(str, knobs)) + "\n" for knobs, _ in CASES)
    out = subprocess.run([str(exe)], input=stdin, capture_output=True,
                         text=True, check=True).stdout.splitlines()
    return out


def _fmt(expected):
    if expected[0] == "reject":
        return "reject %s %d" % expected[1:]
    return ",".join(map(str, expected))


def test_variant_list_is_the_twelve(selected):
    listed = selected[0].split()
    want = {_fmt(e) for _, e in CASES[:12]}
    assert len(listed) == 12 and set(listed) == want


def test_defaults(selected):
    assert selected[1] == "0,1,512,2,0"


@pytest.mark.parametrize("i", range(len(CASES)),
                         ids=["-".join(map(str, k)) for k, _ in CASES])
def test_select(selected, i):
    knobs, expected = CASES[i]
    assert selected[2 + i] == _fmt(expected), knobs
