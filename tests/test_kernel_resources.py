"""Register / scratch budgets of the hot kernels, read from the built gfx950 code object
(tools/kres.py: the AMDGPU metadata of build/csrc/trt_kernel.o, no GPU needed).  A change that
makes the 96-VGPR (5-wave) kernels spill much more shows up here before it costs a GPU run:
the C2 kernel has no scratch at all, the C4 kernel stays near its measured spill level."""
from __future__ import annotations

import re

import pytest

from tests.kres_common import OBJ, kres


@pytest.fixture(scope="module")
def resources():
    if not OBJ.exists():
        pytest.skip("build/csrc/trt_kernel.o not built")
    return {m.group(1): r for name, r in kres("trace_kernel").items()
            if (m := re.fullmatch(r"void trt::trace_kernel<([^>]*)>\(trt::KArgs\)", name))}


def test_c2_kernel_has_no_scratch(resources):
    """The headline kernel (C2: depth 4, no triangles, plain launches): 5 waves, no spills."""
    r = resources["3, false, 0, false, false, false"]
    assert r["vgpr"] <= 96 and r["scratch"] == 0, r


def test_c4_kernel_scratch_budget(resources):
    """C4 (depth 4, quantized BVH4): 96 VGPRs, the private segment stack (96 B) and the
    traversal stack tail (192 B) plus the measured spill slots: 432 B in rounds 5 and 6, the
    budget exactly (a build that spills more fails; the spill-free 4-wave build is 9 % slower,
    DESIGN §7)."""
    r = resources["3, false, 3, false, false, false"]
    assert r["vgpr"] <= 96 and r["scratch"] <= 432, r


def test_lds_fits_the_wave_targets(resources):
    """LDS per one-wave workgroup times the waves per CU the launch bounds ask for stays within
    the 160 KB of a gfx950 CU for the plain and deferred kernels."""
    for key, waves in (("3, false, 0, false, false, false", 20), ("3, false, 3, false, false, false", 20),
                       ("0, false, 3, false, true, false", 16)):
        assert resources[key]["lds"] * waves <= 160 * 1024, (key, resources[key])
