"""Register / scratch budgets of the kernels the sky table adds or touches, read from the built
gfx950 code object (tools/kres.py, no GPU needed): sky_trace_kernel (the plain triangle-free
frame with the sky test and the root-hit form of cast_seg), the plain triangle-free
trace_kernel instantiations it stands in for, and the table's build kernel.  The 5-wave kernels
must stay within 96 VGPRs, and those without a private segment stack (max_depth <= 5) must have
no scratch at all: when the by-value KArgs copy is not folded away (csrc/Makefile KARGFLAGS) the
whole struct lives in scratch and a frame is ~20x slower."""
from __future__ import annotations

import re
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
OBJ = REPO / "build" / "csrc" / "trt_kernel.o"

# trace_kernel<CAP, COUNT, GEOM, SPLIT, DEFER, HYB>: the plain GEOM 0 launches (trt_kernel.hip
# launch_trace) by their deferred-stack capacity; CAP <= 4 keeps the stack in LDS.
PLAIN_G0 = (0, 1, 2, 3, 4, 7, 19)


@pytest.fixture(scope="module")
def resources():
    # a missing object is a failed or skipped kernel build, not a missing GPU: fail, do not skip
    assert OBJ.exists(), "build/csrc/trt_kernel.o is missing: run __graft_entry__.build() first"
    out = subprocess.run([sys.executable, str(REPO / "tools" / "kres.py"), "trace_kernel|sky_kernel"], check=True,
                         capture_output=True, text=True).stdout
    res = {}
    for line in out.splitlines():
        m = re.match(r"(?:void )?trt::(\w+)(?:<([^>]*)>)?\(.*?\)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)", line)
        if m:
            res[(m.group(1), m.group(2))] = dict(vgpr=int(m.group(3)), sgpr=int(m.group(4)), scratch=int(m.group(5)))
    assert res, out[:500]
    return res


@pytest.mark.parametrize("cap", PLAIN_G0)
@pytest.mark.parametrize("kernel", ["sky_trace_kernel", "trace_kernel"])
def test_plain_triangle_free_kernels(resources, kernel, cap):
    r = resources[(kernel, str(cap) if kernel == "sky_trace_kernel" else f"{cap}, false, 0, false, false, false")]
    assert r["vgpr"] <= 96, r
    if cap <= 4:
        assert r["scratch"] == 0, r
    else:  # only the private stack of deep trees: `cap` segments of 8 floats and its index
        assert r["scratch"] <= 32 * cap + 4, r


def test_sky_build_kernel(resources):
    r = resources[("sky_kernel", None)]
    assert r["scratch"] == 0, r
