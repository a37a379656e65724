"""Register / scratch / LDS budgets of sky_trace_kernel_floor<CAP>, the mask kernel with the floor
class, read from the built gfx950 code object (tools/kres.py, no GPU needed).  The floor path is
straight-line code beside trace_tile and must not cost the kernel its 5 waves per SIMD (<= 96
VGPRs) or push KArgs into scratch (no scratch at all for CAP <= 4), and it uses no more LDS than
sky_trace_kernel of the same CAP."""
from __future__ import annotations

import re
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
OBJ = REPO / "build" / "csrc" / "trt_kernel.o"
PLAIN_G0 = (0, 1, 2, 3, 4, 7, 19)


@pytest.fixture(scope="module")
def resources():
    # a missing object is a failed or skipped kernel build, not a missing GPU: fail, do not skip
    assert OBJ.exists(), "build/csrc/trt_kernel.o is missing: run __graft_entry__.build() first"
    out = subprocess.run([sys.executable, str(REPO / "tools" / "kres.py"), "sky_trace_kernel"], check=True,
                         capture_output=True, text=True).stdout
    res = {}
    for line in out.splitlines():
        m = re.match(r"(?:void )?trt::(\w+)<(\d+)>\(.*?\)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+lds\s+(\d+)", line)
        if m:
            res[(m.group(1), int(m.group(2)))] = dict(vgpr=int(m.group(3)), sgpr=int(m.group(4)),
                                                      scratch=int(m.group(5)), lds=int(m.group(6)))
    assert res, out[:500]
    return res


@pytest.mark.parametrize("cap", PLAIN_G0)
def test_sky_trace_kernel_floor_budget(resources, cap):
    r = resources[("sky_trace_kernel_floor", cap)]
    base = resources[("sky_trace_kernel", cap)]
    assert r["vgpr"] <= 96, r
    assert r["sgpr"] <= 106, r
    assert r["lds"] <= base["lds"], (r, base)
    if cap <= 4:
        assert r["scratch"] == 0, r
    else:  # only the private stack of deep trees: `cap` segments of 8 floats and its index
        assert r["scratch"] <= 32 * cap + 4, r
