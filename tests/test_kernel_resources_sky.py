"""Register / scratch budgets of the kernels the sky table adds or touches, read from the built
gfx950 code object (tools/kres.py, no GPU needed): sky_trace_kernel (the plain triangle-free
frame with the sky test and the root-hit form of cast_seg), the plain triangle-free
trace_kernel instantiations it stands in for, and the table's build kernel.  The 5-wave kernels
must stay within 96 VGPRs, and those without a private segment stack (max_depth <= 5) must have
no scratch at all: when the by-value KArgs copy is not folded away (csrc/Makefile KARGFLAGS) the
whole struct lives in scratch and a frame is ~20x slower."""
from __future__ import annotations

import re

import pytest

from tests.kres_common import OBJ, kres

# trace_kernel<CAP, COUNT, GEOM, SPLIT, DEFER, HYB>: the plain GEOM 0 launches (trt_kernel.hip
# launch_trace) by their deferred-stack capacity; CAP <= 4 keeps the stack in LDS.
PLAIN_G0 = (0, 1, 2, 3, 4, 7, 19)


@pytest.fixture(scope="module")
def resources():
    # a missing object is a failed or skipped kernel build, not a missing GPU: fail, do not skip
    assert OBJ.exists(), "build/csrc/trt_kernel.o is missing: run __graft_entry__.build() first"
    return {(m.group(1), m.group(2)): r for name, r in kres("trace_kernel|sky_kernel").items()
            if (m := re.fullmatch(r"(?:void )?trt::(\w+)(?:<([^>]*)>)?\(.*\)", name))}


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
