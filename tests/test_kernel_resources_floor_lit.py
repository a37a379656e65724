"""Register / scratch / LDS budgets of sky_trace_kernel_floor_lit<CAP>, the floor-class kernel of a
grey floor lit from above, and of sky_trace_kernel_floor<CAP> beside it, read
from the built gfx950 code object (tools/kres.py, no GPU needed).  Both keep 5 waves per SIMD
(<= 96 VGPRs), no scratch for CAP <= 4 and no more LDS than sky_trace_kernel of the same CAP.  The
lit kernel's floor path drops two of three colour channels and gains a second, short light loop:
its code stays within 1 KB of the floor kernel's (59,544 against 59,980 bytes for CAP 3)."""
from __future__ import annotations

import re

import pytest

from tests.kres_common import OBJ, kres

PLAIN_G0 = (0, 1, 2, 3, 4, 7, 19)
KERNELS = ("sky_trace_kernel_floor", "sky_trace_kernel_floor_lit")


@pytest.fixture(scope="module")
def resources():
    # a missing object is a failed or skipped kernel build, not a missing GPU: fail, do not skip
    assert OBJ.exists(), "build/csrc/trt_kernel.o is missing: run __graft_entry__.build() first"
    return {(m.group(1), int(m.group(2))): r for name, r in kres("sky_trace_kernel").items()
            if (m := re.fullmatch(r"(?:void )?trt::(\w+)<(\d+)>\(.*\)", name))}


@pytest.mark.parametrize("cap", PLAIN_G0)
@pytest.mark.parametrize("kernel", KERNELS)
def test_budget(resources, kernel, cap):
    r = resources[(kernel, cap)]
    base = resources[("sky_trace_kernel", cap)]
    assert r["vgpr"] <= 96, r
    assert r["sgpr"] <= 106, r
    assert r["spill"] == 0, r
    assert r["lds"] <= base["lds"], (r, base)
    if cap <= 4:
        assert r["scratch"] == 0, r
    else:  # only the private stack of deep trees: `cap` segments of 8 floats and its index
        assert r["scratch"] <= 32 * cap + 4, r


@pytest.mark.parametrize("cap", PLAIN_G0)
def test_lit_kernel_code_size(resources, cap):
    """The sky kernels were cut to one call site per body to fit the instruction cache
    (DESIGN.md 4.23): the lit kernel must not grow back."""
    lit, floor = resources[("sky_trace_kernel_floor_lit", cap)], resources[("sky_trace_kernel_floor", cap)]
    assert lit["code"] <= floor["code"] + 1024, (lit, floor)
