"""Register / scratch / LDS budgets of the kernels the sky spans change or add, read from the built
gfx950 code object (tools/kres.py, no GPU needed).  sky_trace_kernel<CAP> gained the span test
(scalar work on the wave-uniform tile) and the culled tile's store; sky_trace_kernel_nospan<CAP>
is the kernel without them, for launches that carry no spans.  Both must keep 5 waves per SIMD
(<= 96 VGPRs), keep KArgs — now 3.9 KB with the span words — out of scratch (no scratch at all
for CAP <= 4), and use no more LDS than the plain trace_kernel of the same CAP.  The span words
ride in every kernel's arguments, so the plain trace_kernel instantiations, which never read
them, are checked for the same budgets (profiles/sky_spans_kres.txt lists every kernel before
and after)."""
from __future__ import annotations

import re

import pytest

from tests.kres_common import OBJ, kres

PLAIN_G0 = (0, 1, 2, 3, 4, 7, 19)


@pytest.fixture(scope="module")
def resources():
    # a missing object is a failed or skipped kernel build, not a missing GPU: fail, do not skip
    assert OBJ.exists(), "build/csrc/trt_kernel.o is missing: run __graft_entry__.build() first"
    return {(m.group(1), m.group(2)): r for name, r in kres("trace_kernel").items()
            if (m := re.fullmatch(r"(?:void )?trt::(\w+)(?:<([^>]*)>)?\(.*\)", name))}


@pytest.mark.parametrize("cap", PLAIN_G0)
@pytest.mark.parametrize("kernel", ["sky_trace_kernel", "sky_trace_kernel_nospan"])
def test_sky_trace_kernel_budget(resources, kernel, cap):
    r = resources[(kernel, str(cap))]
    plain = resources[("trace_kernel", f"{cap}, false, 0, false, false, false")]
    assert r["vgpr"] <= 96, r
    assert r["sgpr"] <= 106, r
    assert r["lds"] <= plain["lds"], (r, plain)
    assert plain["vgpr"] <= 96, plain
    if cap <= 4:
        assert r["scratch"] == 0 and plain["scratch"] == 0, (r, plain)
    else:  # only the private stack of deep trees: `cap` segments of 8 floats and its index
        assert r["scratch"] <= 32 * cap + 4, r
