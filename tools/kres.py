#!/usr/bin/env python3
"""Kernel resources (VGPRs, SGPRs, scratch bytes per lane, LDS) of the built trace kernels, read
from the gfx950 code object inside build/csrc/trt_kernel.o (llvm-objdump --offloading + the
AMDGPU metadata notes): `make resources` without a recompile.  `code` is the kernel's symbol
size in bytes (its instructions: what it asks of the instruction cache).

    python tools/kres.py [regex [object]]     (default: every trace/defer kernel of the build)

Second mode, the gate of a refactor of trt_kernel.hip: two device assemblies of it
(hipcc --cuda-device-only -S with the flags of `make print-kernel-flags`) compared kernel by kernel.

    python tools/kres.py --diff A.s B.s

    (a) identical: the instruction text (comments and directives stripped) and the resource fields
        of the metadata are equal;
    (b) the instructions differ, the resources are equal or only the SGPR count is lower in B;
    (c) anything else: more of a resource in B, or fewer VGPRs / scratch / LDS / spills (a change
        worth a look of its own).
Kernels present on one side only are listed.  No instruction is interpreted: text against text.
"""
from __future__ import annotations

import re
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
LLVM = Path("/opt/rocm/lib/llvm/bin")
# metadata field -> the short name of the listing
FIELDS = {"vgpr_count": "vgpr", "sgpr_count": "sgpr", "private_segment_fixed_size": "scratch",
          "group_segment_fixed_size": "lds", "vgpr_spill_count": "spill_v"}


def metadata(text: str) -> dict[str, dict[str, int]]:
    """{mangled kernel name: {short field name: value}} of an AMDGPU metadata document, as
    llvm-readelf --notes prints it and as the assembly's .amdgpu_metadata block holds it."""
    out = {}
    for blk in re.split(r"\n  - \.agpr_count", text)[1:]:
        def g(k):
            return re.search(r"\." + k + r":\s+(\S+)", blk).group(1)
        out[g("name")] = {short: int(g(k)) for k, short in FIELDS.items()}
    return out


def demangle(names: list[str]) -> list[str]:
    return subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                          check=True).stdout.splitlines()


def resources(pattern: str, obj: Path | None = None) -> dict[str, dict[str, int]]:
    """{demangled kernel name: vgpr, sgpr, scratch, lds, spill_v, code} of the kernels of the built
    object whose mangled name matches `pattern`."""
    pat = re.compile(pattern)
    obj = obj or REPO / "build" / "csrc" / "trt_kernel.o"
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
    meta = {n: r for n, r in metadata(notes).items() if pat.search(n)}
    return {d: dict(r, code=size[n]) for d, (n, r) in zip(demangle(list(meta)), meta.items())}


def instructions(path: str) -> dict[str, list[str]]:
    """{mangled function name: its instruction and label lines} of a device assembly."""
    fns, cur, buf = {}, None, []
    for ln in open(path):
        if cur is None:
            m = re.match(r"(_Z\w+):", ln)
            if m:
                cur, buf = m.group(1), []
        elif ln.startswith(".Lfunc_end"):
            fns[cur], cur = buf, None
        else:
            s = ln.split(";")[0].strip()
            if s and (not s.startswith(".") or s.startswith(".LBB")):
                buf.append(re.sub(r"\.LBB\d+_", ".LBB_", s))  # block labels without the function's ordinal
    return fns


def diff(path_a: str, path_b: str) -> None:
    ia, ib = instructions(path_a), instructions(path_b)
    ma, mb = metadata(open(path_a).read()), metadata(open(path_b).read())
    both = [k for k in ma if k in mb]
    name = dict(zip(ma.keys() | mb.keys(), demangle(list(ma.keys() | mb.keys()))))
    cls = {"a": [], "b": [], "c": []}
    for k in both:
        ra, rb = ma[k], mb[k]
        rest_equal = all(ra[f] == rb[f] for f in ra if f != "sgpr")
        if ia[k] == ib[k] and ra == rb:
            cls["a"].append(k)
        elif rest_equal and rb["sgpr"] <= ra["sgpr"]:
            cls["b"].append(k)
        else:
            cls["c"].append(k)
    print(f"{len(both)} kernels on both sides: (a) identical {len(cls['a'])}, (b) resources equal or SGPRs lower "
          f"{len(cls['b'])}, (c) other {len(cls['c'])}")
    for c in ("b", "c"):
        for k in sorted(cls[c], key=name.get):
            d = " ".join(f"{f} {ma[k][f]}->{mb[k][f]}" for f in ma[k] if ma[k][f] != mb[k][f])
            print(f"({c}) {name[k]}: lines {len(ia[k])}->{len(ib[k])} {d}")
    for side, here, there in (("A", ma, mb), ("B", mb, ma)):
        for k in sorted(set(here) - set(there), key=name.get):
            print(f"only in {side}: {name[k]}")
    for k in sorted(cls["a"], key=name.get):
        print(f"(a) {name[k]}")


def main() -> None:
    if len(sys.argv) == 4 and sys.argv[1] == "--diff":
        return diff(sys.argv[2], sys.argv[3])
    res = resources(sys.argv[1] if len(sys.argv) > 1 else r"trace_|defer_", Path(sys.argv[2]) if len(sys.argv) > 2 else None)
    for dem, r in res.items():
        print(f"{dem:70s} vgpr {r['vgpr']:>4} sgpr {r['sgpr']:>4} scratch {r['scratch']:>5} "
              f"lds {r['lds']:>6} spill_v {r['spill_v']} code {r['code']:>6}")


if __name__ == "__main__":
    main()
