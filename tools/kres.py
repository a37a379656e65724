#!/usr/bin/env python3
"""Kernel resources (VGPRs, SGPRs, scratch bytes per lane, LDS) of the built trace kernels, read
from the gfx950 code object inside build/csrc/trt_kernel.o (llvm-objdump --offloading + the
AMDGPU metadata notes): `make resources` without a recompile.  `code` is the kernel's symbol
size in bytes (its instructions: what it asks of the instruction cache).

    python tools/kres.py [regex [object]]     (default: every trace/defer kernel of the build)
"""
from __future__ import annotations

import re
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
LLVM = Path("/opt/rocm/lib/llvm/bin")


def main() -> None:
    pat = re.compile(sys.argv[1] if len(sys.argv) > 1 else r"trace_|defer_")
    obj = Path(sys.argv[2]) if len(sys.argv) > 2 else REPO / "build" / "csrc" / "trt_kernel.o"
    with tempfile.TemporaryDirectory() as td:
        tmp = Path(td) / "k.o"
        tmp.write_bytes(obj.read_bytes())
        subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(tmp)], check=True, capture_output=True)
        co = next(Path(td).glob("k.o.*gfx950*"))
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True,
                               text=True).stdout
        syms = subprocess.run([str(LLVM / "llvm-readelf"), "--symbols", "--wide", str(co)], check=True,
                              capture_output=True, text=True).stdout
    size = {}  # FUNC symbols: Num Value Size Type Bind Vis Ndx Name
    for ln in syms.splitlines():
        w = ln.split()
        if len(w) == 8 and w[3] == "FUNC":
            size[w[7]] = int(w[2], 0)
    for blk in re.split(r"\n  - \.agpr_count", notes)[1:]:
        def g(k):
            m = re.search(r"\." + k + r":\s+(\S+)", blk)
            return m.group(1) if m else "?"
        name = g("name")
        if not pat.search(name):
            continue
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        print(f"{dem:70s} vgpr {g('vgpr_count'):>4} sgpr {g('sgpr_count'):>4} scratch {g('private_segment_fixed_size'):>5} "
              f"lds {g('group_segment_fixed_size'):>6} spill_v {g('vgpr_spill_count')} code {size.get(name, '?'):>6}")


if __name__ == "__main__":
    main()
