"""Register / scratch / LDS budgets of sky_trace_kernel_floor<CAP>, the mask kernel with the floor
class, read from the built gfx950 code object (tools/kres.py, no GPU needed).  The floor path is
straight-line code beside trace_tile and must not cost the kernel its 5 waves per SIMD (<= 96
VGPRs) or push KArgs into scratch (no scratch at all for CAP <= 4), and it uses no more LDS than
sky_trace_kernel of the same CAP."""
from __future__ import annotations

import re

import pytest

from tests.kres_common import OBJ, kres

PLAIN_G0 = (0, 1, 2, 3, 4, 7, 19)


@pytest.fixture(scope="module")
def resources():
    # a missing object is a failed or skipped kernel build, not a missing GPU: fail, do not skip
    assert OBJ.exists(), "build/csrc/trt_kernel.o is missing: run __graft_entry__.build() first"
    return {(m.group(1), int(m.group(2))): r for name, r in kres("sky_trace_kernel").items()
            if (m := re.fullmatch(r"(?:void )?trt::(\w+)<(\d+)>\(.*\)", name))}


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
