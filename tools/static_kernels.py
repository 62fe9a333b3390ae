#!/usr/bin/env python3
"""Compare the kernels of two builds from their compiler-generated assembly.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -DNDEBUG -S --cuda-device-only \
        burst_attn_amd/csrc/attn_fwd.hip -o new/attn_fwd.s      (same for bwd,
        and for the parent commit's sources into parent/)
    python tools/static_kernels.py parent/ new/

Every kernel of the parent must be in the new build with the same
instructions once symbol names and block-label numbers are normalised (a
kernel whose template gained a trailing empty parameter pack keeps its
identity).  New kernels are listed with their resources.  Needs no GPU.
"""

import glob
import os
import re
import sys

RES = {
    "vgpr": r"; NumVgprs: (\d+)",
    "agpr": r"; NumAgprs: (\d+)",
    "scratch": r"; ScratchSize: (\d+)",
    "lds": r"; LDSByteSize: (\d+)",
    "occ": r"; Occupancy: (\d+)",
    "code": r"; codeLenInByte = (\d+)",
}


def key_of(name):
    """Template part of a mangled kernel name, empty trailing pack dropped."""
    k = name.split("EEvP")[0] if "EEvP" in name else name
    return k[:-2] if k.endswith("JE") else k


def kernels(path):
    out = {}
    for f in sorted(glob.glob(os.path.join(path, "*.s"))):
        text = open(f).read()
        for m in re.finditer(r"^(\S+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:\n",
                             text, re.S | re.M):
            name, body = m.groups()
            if ".amdhsa_kernel " + name + "\n" not in text:
                continue
            # the resource comments follow the function, before the next one
            tail = text[m.end():].split("; -- Begin function")[0]
            insts = []
            for line in body.split("\n"):
                line = line.split(";")[0].strip()
                if not line or line.startswith(".") or line.endswith(":"):
                    continue
                line = re.sub(r"_Z\w+", "SYM", line)
                line = re.sub(r"\.LBB\d+_", ".LBB_", line)
                insts.append(line)
            res = {k: int(re.search(p, tail).group(1)) if re.search(p, tail)
                   else -1 for k, p in RES.items()}
            out[key_of(name)] = (insts, res)
    return out


def main(parent_dir, new_dir):
    old, new = kernels(parent_dir), kernels(new_dir)
    same = [k for k in old if k in new and old[k][0] == new[k][0]]
    differ = [k for k in old if k in new and old[k][0] != new[k][0]]
    missing = [k for k in old if k not in new]
    for k in sorted(new):
        if k in old and k not in differ:
            continue
        insts, r = new[k]
        tag = "(differs from parent: %d inst there)" % len(old[k][0]) \
            if k in old else "(new)"
        print("%s: inst %d vgpr %d agpr %d scratch %d lds %d occ %d code %d  %s"
              % (k, len(insts), r["vgpr"], r["agpr"], r["scratch"], r["lds"],
                 r["occ"], r["code"], tag))
    print("old kernels identical: %d, differing: %d, parent kernels: %d, "
          "change kernels: %d, missing: %s"
          % (len(same), len(differ), len(old), len(new), missing or "none"))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
