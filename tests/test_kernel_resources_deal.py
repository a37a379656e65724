"""Register, scratch and code-size budgets of the five sky kernels with the host's dealing
constants and magic divisors (KArgs::deal, csrc/trt_deal.h), read from the built
gfx950 code object (tools/kres.py, no GPU needed).  The
kernels must stay at 5 waves per SIMD (<= 96 VGPRs: 512 / 96 = 5) without scratch for CAP <= 4,
and sky_trace_kernel_floor_lit<3>, the kernel of the C2 headline, within 65,536 bytes of code.
One more use of the by-value KArgs that the compiler cannot fold (a pointer into it kept across
trace_body's branches) puts the 4 KB copy into scratch: the scratch assertion is what catches
that.  Sizes and resource notes only: no instruction is read."""
from __future__ import annotations

import re

import pytest

from tests.kres_common import OBJ, kres

KERNELS = ("sky_trace_kernel_floor_lit", "sky_trace_kernel_floor", "sky_trace_kernel_smask", "sky_trace_kernel",
           "sky_trace_kernel_nospan")
CAPS = (0, 1, 2, 3, 4)
VGPRS_PER_SIMD_LANE = 512  # gfx950: 512 VGPRs per lane of a SIMD, allocated in blocks of 8


@pytest.fixture(scope="module")
def resources():
    # a missing object is a failed or skipped kernel build, not a missing GPU: fail, do not skip
    assert OBJ.exists(), "build/csrc/trt_kernel.o is missing: run __graft_entry__.build() first"
    return {(m.group(1), int(m.group(2))): r for name, r in kres("sky_trace_kernel").items()
            if (m := re.fullmatch(r"(?:void )?trt::(\w+)<(\d+)>\(.*\)", name))}


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("cap", CAPS)
def test_sky_kernel_budget(resources, kernel, cap):
    r = resources[(kernel, cap)]
    assert r["vgpr"] <= 96, r
    assert r["scratch"] == 0 and r["spill"] == 0, r
    alloc = -(-r["vgpr"] // 8) * 8
    assert min(8, VGPRS_PER_SIMD_LANE // alloc) == 5, r  # occupancy: the launch bound asks for 5 waves per SIMD


def test_headline_kernel_fits_the_instruction_cache(resources):
    r = resources[("sky_trace_kernel_floor_lit", 3)]
    assert 0 < r["code"] <= 65536, r
