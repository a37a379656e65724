"""Register / scratch / LDS budget of visibility_query_kernel<GEOM> (abi.h trt_visibility), read from
the built gfx950 code object (tools/kres.py, no GPU needed).

The yardstick is occlusion_query_kernel<GEOM> in the same object: the kernel that runs the same
any-hit walk (shadow_intersect<false, GEOM>) over caller-made segments.  The visibility kernel forms
its segment (the point predicate, the flip or the target difference and its square root) before the
walk, where register pressure is lowest, and its ballot and mask store come after it, so it must
need no more scratch and no more LDS than its yardstick and must fit the occupancy its
__launch_bounds__ ask for (the same waves_per_simd<GEOM>()).  GEOM 3 has two instantiations: with
the wave-cooperative shadow walk behind shadow_intersect's gate (COOP, as the yardstick) and
without it (the default); both are held to the same budget, and there are no others."""
from __future__ import annotations

import re

import pytest

from tests.kres_common import OBJ, REPO, kres

KERNEL_SRC = REPO / "vkcomputeshader_tinyraytracer_amd" / "csrc" / "trt_kernel.hip"


def _kres(kernel: str, variants: list) -> dict:
    """{template arguments as written: resources} of `kernel`'s instantiations, which must be exactly `variants`."""
    res = {m.group(1): r for name, r in kres(kernel).items()
           if (m := re.fullmatch(rf"void trt::{kernel}<([^>]*)>\(trt::KArgs.*\)", name))}
    assert sorted(res) == sorted(variants), res
    return res


VARIANTS = {"0, true": 0, "1, true": 1, "2, true": 2, "3, true": 3, "3, false": 3}  # <GEOM, COOP> -> GEOM


@pytest.fixture(scope="module")
def resources():
    if not OBJ.exists():
        pytest.skip("build/csrc/trt_kernel.o not built")
    return _kres("visibility_query_kernel", list(VARIANTS)), _kres("occlusion_query_kernel", ["0", "1", "2", "3"])


def _define(src: str, name: str) -> int:
    m = re.search(rf"#define {name} (\d+)\b", src)
    assert m, name
    return int(m.group(1))


def vgpr_cap(geom: int) -> int:
    """The VGPRs a wave may hold at waves_per_simd<GEOM>() waves per SIMD (CAP = 99): 512 per SIMD
    lane, allocated in blocks of 8."""
    src = KERNEL_SRC.read_text()
    assert "__launch_bounds__(64, waves_per_simd<GEOM>()) void visibility_query_kernel(" in src
    assert "return GEOM == 3 ? (CAP <= 3 ? TRT_G3_WAVES_SHALLOW : TRT_G3_WAVES) : GEOM == 0 ? TRT_G0_WAVES : TRT_WAVES;" in src
    waves = _define(src, "TRT_G3_WAVES" if geom == 3 else "TRT_G0_WAVES" if geom == 0 else "TRT_WAVES")
    assert 1 <= waves <= 8
    return (512 // waves) // 8 * 8


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_no_more_than_the_occlusion_query_kernel(resources, variant):
    vis, yard = resources
    geom = VARIANTS[variant]
    r, y = vis[variant], yard[str(geom)]
    print(f"<{variant}>: visibility_query_kernel {r}, occlusion_query_kernel {y}, VGPR cap {vgpr_cap(geom)}")
    assert r["scratch"] <= y["scratch"], (r, y)
    assert r["lds"] <= y["lds"], (r, y)
    assert r["vgpr"] <= vgpr_cap(geom), (r, vgpr_cap(geom))


def test_triangle_free_kernel_has_no_scratch(resources):
    assert resources[0]["0, true"]["scratch"] == 0, resources[0]["0, true"]
