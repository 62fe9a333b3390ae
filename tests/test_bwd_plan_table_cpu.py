"""CPU checks of the backward launch layer.

The plan table (burst_attn_amd/csrc/bwd_plans.h) is host-only, so a plain
C++ compiler builds it with a small main that prints what ba_bwd_select
returns for a list of (fused, dk_flip, dq_pipe, dkq_dbg, G) tuples.  The
expected step lists below are transcribed from the if-ladder the table
replaced, not from the header.  That ladder was:

    G > 1 and FUSED in {1,2}      -> unsupported, names BA_BWD_FUSED
    G > 1 and DK_FLIP             -> unsupported, names BA_BWD_DK_FLIP
    FUSED != 2                    -> launch dq (DQP = DQ_PIPE)
    FUSED == 1                    -> launch fused dK+dV, done
    otherwise                     -> launch split dV
    FUSED == 2                    -> launch atomic dK+dQ (DBG 1, 2, else 0)
    else DK_FLIP                  -> launch flipped dK
    else                          -> launch split dK

The second test only checks that tools/dkq_probe.hip, which launches the
kernels through attn_bwd.hip's argument structs, still compiles.
"""

import itertools
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "burst_attn_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

MAIN = r"""
#include <stdio.h>
#include "bwd_plans.h"
// stdin: one "fused dk_flip dq_pipe dkq_dbg G" tuple per line; stdout: the
// step names ba_bwd_select lists, or the verdict.  First line: the defaults.
static const char* name(ba_bwd_step s) {
  switch (s) {
    case BA_STEP_DQ: return "dq";
    case BA_STEP_DQ_PIPE: return "dq_pipe";
    case BA_STEP_DV: return "dv";
    case BA_STEP_DK: return "dk";
    case BA_STEP_DK_FLIPPED: return "dk_flipped";
    case BA_STEP_DKDV_FUSED: return "dkdv_fused";
    case BA_STEP_DKDQ_ATOMIC: return "dkdq_atomic";
    case BA_STEP_DKDQ_DBG1: return "dkdq_dbg1";
    case BA_STEP_DKDQ_DBG2: return "dkdq_dbg2";
  }
  return "?";
}
int main() {
  ba_bwd_knobs k;
  int G;
  printf("%d %d %d %d\n", k.fused, k.dk_flip, k.dq_pipe, k.dkq_dbg);
  while (scanf("%d %d %d %d %d", &k.fused, &k.dk_flip, &k.dq_pipe,
               &k.dkq_dbg, &G) == 5) {
    const ba_bwd_plan p = ba_bwd_select(k, G);
    if (p.verdict == BA_BWD_BAD_VALUE)
      printf("reject %s %d", p.knob, p.value);
    else if (p.verdict == BA_BWD_NO_GQA)
      printf("no_gqa %s %d", p.knob, p.value);
    for (int i = 0; i < p.n_steps; ++i) printf("%s ", name(p.steps[i]));
    printf("\n");
  }
  return 0;
}
"""


# (fused, dk_flip, dq_pipe, G) -> expected output line for every dkq_dbg;
# only the atomic dK+dQ step depends on it ("{dkdq}").
ATOMIC = {0: "dkdq_atomic", 1: "dkdq_dbg1", 2: "dkdq_dbg2"}
TABLE = {
    (0, 0, 0, 1): "dq dv dk",
    (0, 0, 1, 1): "dq_pipe dv dk",
    (0, 1, 0, 1): "dq dv dk_flipped",
    (0, 1, 1, 1): "dq_pipe dv dk_flipped",
    (1, 0, 0, 1): "dq dkdv_fused",
    (1, 0, 1, 1): "dq_pipe dkdv_fused",
    (1, 1, 0, 1): "dq dkdv_fused",
    (1, 1, 1, 1): "dq_pipe dkdv_fused",
    (2, 0, 0, 1): "dv {dkdq}",
    (2, 0, 1, 1): "dv {dkdq}",
    (2, 1, 0, 1): "dv {dkdq}",
    (2, 1, 1, 1): "dv {dkdq}",
    (0, 0, 0, 4): "dq dv dk",
    (0, 0, 1, 4): "dq_pipe dv dk",
    (0, 1, 0, 4): "no_gqa BA_BWD_DK_FLIP 1",
    (0, 1, 1, 4): "no_gqa BA_BWD_DK_FLIP 1",
    (1, 0, 0, 4): "no_gqa BA_BWD_FUSED 1",
    (1, 0, 1, 4): "no_gqa BA_BWD_FUSED 1",
    (1, 1, 0, 4): "no_gqa BA_BWD_FUSED 1",
    (1, 1, 1, 4): "no_gqa BA_BWD_FUSED 1",
    (2, 0, 0, 4): "no_gqa BA_BWD_FUSED 2",
    (2, 0, 1, 4): "no_gqa BA_BWD_FUSED 2",
    (2, 1, 0, 4): "no_gqa BA_BWD_FUSED 2",
    (2, 1, 1, 4): "no_gqa BA_BWD_FUSED 2",
}
# (fused, dk_flip, dq_pipe, dkq_dbg, G) -> expected output line
GRID = [((f, fl, p, dbg, g), TABLE[f, fl, p, g].format(dkdq=ATOMIC[dbg]))
        for f, fl, p, dbg, g in itertools.product(
            (0, 1, 2), (0, 1), (0, 1), (0, 1, 2), (1, 4))]
REJECTS = [
    # one rejected value per knob; a bad value beats the GQA check
    ((3, 0, 0, 0, 1), "reject BA_BWD_FUSED 3"),
    ((-1, 0, 0, 0, 1), "reject BA_BWD_FUSED -1"),
    ((0, 2, 0, 0, 1), "reject BA_BWD_DK_FLIP 2"),
    ((0, 0, 2, 0, 1), "reject BA_DQ_PIPE 2"),
    ((0, 0, 0, 3, 1), "reject BA_DKQ_DBG 3"),
    ((1, 0, 0, 3, 4), "reject BA_DKQ_DBG 3"),
]
CASES = GRID + REJECTS


@pytest.fixture(scope="module")
def selected(tmp_path_factory):
    if shutil.which("c++"):
        cc = ["c++"]
    elif shutil.which(HIPCC):
        cc = [HIPCC, "-x", "c++"]
    else:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("bwd_plans")
    src, exe = d / "main.cpp", d / "main"
    src.write_text(MAIN)
    subprocess.run(cc + ["-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                         str(src), "-o", str(exe)], check=True)
    stdin = "".join(" ".join(map(str, knobs)) + "\n" for knobs, _ in CASES)
    out = subprocess.run([str(exe)], input=stdin, capture_output=True,
                         text=True, check=True).stdout.splitlines()
    return [line.strip() for line in out]


def test_grid_is_the_72_combinations():
    assert len(GRID) == 72 and len({k for k, _ in GRID}) == 72


def test_defaults(selected):
    assert selected[0] == "0 0 0 0"


@pytest.mark.parametrize("i", range(len(CASES)),
                         ids=["_".join(map(str, k)) + f"-{i}"
                              for i, (k, _) in enumerate(CASES)])
def test_select(selected, i):
    knobs, expected = CASES[i]
    assert selected[1 + i] == expected, knobs


def test_dkq_probe_compiles():
    if not shutil.which(HIPCC):
        pytest.skip("no hipcc")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17",
                    "-fsyntax-only",
                    os.path.join(REPO, "tools", "dkq_probe.hip")], check=True)
