"""Register / scratch / LDS budgets of sky_trace_kernel_smask<CAP>, the span kernel with the shadow
occluder masks, read from the built gfx950 code object (tools/kres.py, no GPU needed).  The mask
is one VGPR per lane across the light loop and a few scalar registers; the kernel must keep 5
waves per SIMD (<= 96 VGPRs), keep KArgs out of scratch (no scratch at all for CAP <= 4) and use
no more LDS than sky_trace_kernel of the same CAP, the kernel a launch without masks runs."""
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
def test_sky_trace_kernel_smask_budget(resources, cap):
    r = resources[("sky_trace_kernel_smask", cap)]
    base = resources[("sky_trace_kernel", cap)]
    assert r["vgpr"] <= 96, r
    assert r["sgpr"] <= 106, r
    assert r["lds"] <= base["lds"], (r, base)
    if cap <= 4:
        assert r["scratch"] == 0, r
    else:  # only the private stack of deep trees: `cap` segments of 8 floats and its index
        assert r["scratch"] <= 32 * cap + 4, r
