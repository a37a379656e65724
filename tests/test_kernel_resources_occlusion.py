"""Register / scratch / LDS budget of occlusion_query_kernel<GEOM> (abi.h trt_occluded), read from
the built gfx950 code object (tools/kres.py, no GPU needed).

The yardstick is shadow_batch_kernel<GEOM> in the same object: the existing kernel that runs the
same any-hit walk (shadow_intersect<false, GEOM>) over a dense array.  Validation, the normalize and
the floor test all happen before the walk, where register pressure is lowest, so the query kernel
must need no more scratch and no more LDS than its yardstick, and must fit the occupancy its
__launch_bounds__ ask for (the same waves_per_simd<GEOM>() as the yardstick)."""
from __future__ import annotations

import re

import pytest

from tests.kres_common import OBJ, REPO, kres

KERNEL_SRC = REPO / "vkcomputeshader_tinyraytracer_amd" / "csrc" / "trt_kernel.hip"


def _kres(kernel: str) -> dict:
    res = {int(m.group(1)): r for name, r in kres(kernel).items()
           if (m := re.fullmatch(rf"void trt::{kernel}<(\d)>\(trt::KArgs.*\)", name))}
    assert sorted(res) == [0, 1, 2, 3], res
    return res


@pytest.fixture(scope="module")
def resources():
    if not OBJ.exists():
        pytest.skip("build/csrc/trt_kernel.o not built")
    return _kres("occlusion_query_kernel"), _kres("shadow_batch_kernel")


def _define(src: str, name: str) -> int:
    m = re.search(rf"#define {name} (\d+)\b", src)
    assert m, name
    return int(m.group(1))


def vgpr_cap(geom: int) -> int:
    """The VGPRs a wave may hold at waves_per_simd<GEOM>() waves per SIMD (CAP = 99): 512 per SIMD
    lane, allocated in blocks of 8."""
    src = KERNEL_SRC.read_text()
    assert "__launch_bounds__(64, waves_per_simd<GEOM>()) void occlusion_query_kernel(" in src
    assert "return GEOM == 3 ? (CAP <= 3 ? TRT_G3_WAVES_SHALLOW : TRT_G3_WAVES) : GEOM == 0 ? TRT_G0_WAVES : TRT_WAVES;" in src
    waves = _define(src, "TRT_G3_WAVES" if geom == 3 else "TRT_G0_WAVES" if geom == 0 else "TRT_WAVES")
    assert 1 <= waves <= 8
    return (512 // waves) // 8 * 8


@pytest.mark.parametrize("geom", [0, 1, 2, 3])
def test_no_more_than_the_shadow_batch_kernel(resources, geom):
    occ, yard = resources
    r, y = occ[geom], yard[geom]
    print(f"GEOM {geom}: occlusion_query_kernel {r}, shadow_batch_kernel {y}, VGPR cap {vgpr_cap(geom)}")
    assert r["scratch"] <= y["scratch"], (r, y)
    assert r["lds"] <= y["lds"], (r, y)
    assert r["vgpr"] <= vgpr_cap(geom), (r, vgpr_cap(geom))


def test_triangle_free_kernel_has_no_scratch(resources):
    assert resources[0][0]["scratch"] == 0, resources[0][0]
