"""Register / scratch budgets of the kernels that trace oriented frames (abi.h trt_view), read from
the built gfx950 code object (tools/kres.py, no GPU needed).

Oriented frames are served by the EXISTING trace_kernel instantiations: primary_dir tests the
launch's wave-uniform view_on and, for an oriented launch, turns the host direction with nine
scalar-operand VALU operations before the trace begins, where register pressure is lowest.  So the
keys below are the ones tests/test_kernel_resources.py pins, under the same budgets, plus the
other stack depths a plain triangle-free frame launches (max_depth 1..5: CAP 0..4).  The sky
table's kernels compile primary_dir without the view (they never see one): their budgets are
pinned by tests/test_kernel_resources_sky.py, _spans, _smask and _floor, unchanged."""
from __future__ import annotations

import re

import pytest

from tests.kres_common import OBJ, REPO, kres


@pytest.fixture(scope="module")
def resources():
    if not OBJ.exists():
        pytest.skip("build/csrc/trt_kernel.o not built")
    return {m.group(1): r for name, r in kres("trace_kernel").items()
            if (m := re.fullmatch(r"void trt::trace_kernel<([^>]*)>\(trt::KArgs\)", name))}


@pytest.mark.parametrize("cap", [0, 1, 2, 3, 4])
def test_oriented_triangle_free_kernels_have_no_scratch(resources, cap):
    """Plain GEOM 0 frames (C1 / C2, oriented or not, without the sky table): 5 waves, no spills."""
    r = resources[f"{cap}, false, 0, false, false, false"]
    assert r["vgpr"] <= 96 and r["scratch"] == 0, r


def test_oriented_c4_kernel_scratch_budget(resources):
    """The plain GEOM 3 kernel at CAP 3 (C4), which also traces its oriented frames: the project's
    budget of 96 VGPRs and 432 B of scratch."""
    r = resources["3, false, 3, false, false, false"]
    assert r["vgpr"] <= 96 and r["scratch"] <= 432, r


def test_kernel_arguments_hold_the_views():
    """One launch carries at least 16 oriented frames, each with its own basis, inside the 4 KB
    kernel-argument segment (trt_device.h asserts both at compile time; this reads the header)."""
    src = (REPO / "vkcomputeshader_tinyraytracer_amd" / "csrc" / "trt_device.h").read_text()
    m = re.search(r"constexpr uint32_t kMaxViewFrames = (\d+);", src)
    assert m and int(m.group(1)) >= 16
    assert "sizeof(KArgs) <= 4096" in src
    abi = (REPO / "include" / "trt" / "abi.h").read_text()
    assert f"#define TRT_MAX_VIEW_FRAMES {m.group(1)}u" in abi
