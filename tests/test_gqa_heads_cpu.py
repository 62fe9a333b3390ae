"""CPU check of the grouped-query head mapping the launchers use
(burst_attn_amd/csrc/gqa_heads.h).

The header is host-only, so a plain C++ compiler builds it with a small
main (the pattern of tests/test_fwd_variant_table_cpu.py).  ba_gqa_group is
what fwd_entry and bahip_attn_bwd_gqa call to validate (N, Nk) and derive G; 0 is
the value they turn into BAHIP_ERR_UNSUPPORTED.
"""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "burst_attn_amd", "csrc")

MAIN = r"""
#include <stdio.h>
#include "gqa_heads.h"
static_assert(ba_gqa_group(32, 8) == 4, "usable in constant expressions");
// stdin: one "N Nk" pair per line; stdout: "G:" followed, for a valid pair,
// by the kv head of every q head.
int main() {
  long long N, Nk;
  while (scanf("%lld %lld", &N, &Nk) == 2) {
    const int64_t G = ba_gqa_group(N, Nk);
    printf("%lld:", (long long)G);
    if (G)
      for (int64_t n = 0; n < N; ++n)
        printf(" %lld", (long long)ba_gqa_kv_head(n, G));
    printf("\n");
  }
  return 0;
}
"""

# (N, Nk) -> G (0 = rejected)
CASES = [
    ((32, 8), 4), ((4, 2), 2), ((6, 2), 3), ((4, 1), 4), ((4, 4), 1),
    ((1, 1), 1),
    ((4, 3), 0), ((4, 0), 0), ((4, -2), 0), ((2, 4), 0), ((0, 1), 0),
    ((7, 2), 0),
]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if shutil.which("c++"):
        cc = ["c++"]
    elif shutil.which(hipcc):
        cc = [hipcc, "-x", "c++"]
    else:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("gqa_heads")
    src, exe = d / "main.cpp", d / "main"
    src.write_text(MAIN)
    subprocess.run(cc + ["-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                         str(src), "-o", str(exe)], check=True)
    stdin = "".join(f"{n} {nk}\n" for (n, nk), _ in CASES)
    return subprocess.run([str(exe)], input=stdin, capture_output=True,
                          text=True, check=True).stdout.splitlines()


@pytest.mark.parametrize("i", range(len(CASES)),
                         ids=[f"N{n}-Nk{nk}" for (n, nk), _ in CASES])
def test_group_and_kv_head(lines, i):
    (n, nk), g = CASES[i]
    head, _, rest = lines[i].partition(":")
    assert int(head) == g
    if g:
        # flash-attn convention: query head h attends kv head h // G
        assert [int(x) for x in rest.split()] == [h // g for h in range(n)]
    else:
        assert rest.strip() == ""
