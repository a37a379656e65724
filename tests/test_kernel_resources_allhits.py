"""Register / scratch / LDS budget of all_hits_kernel<GEOM, RECORDS> (abi.h trt_trace_all), read from
the built gfx950 code object (tools/kres.py, no GPU needed).

The yardstick is ray_query_kernel<0, false, GEOM, false> in the same object, the hits-only ray query:
it runs the same nearest-hit walk (scene_intersect<false, GEOM>) and stores the same record.  The
all-hits kernel repeats that search with a lower bound on the candidates' keys and keeps nothing per
hit (each record goes straight to its slot), so it must need no more LDS than its yardstick, no
scratch where there are no triangles, and must fit the occupancy its __launch_bounds__ ask for
(waves_per_simd<GEOM>(), as occlusion_query_kernel).  The mesh walks' scratch is the traversal
stack's private tail; it is printed beside the yardstick's and held to it.  The instantiations are
GEOM 0-3 x {records, counts only}, and there are no others."""
from __future__ import annotations

import re

import pytest

from tests.kres_common import OBJ, REPO, kres

KERNEL_SRC = REPO / "vkcomputeshader_tinyraytracer_amd" / "csrc" / "trt_kernel.hip"
VARIANTS = {f"{g}, {r}": g for g in range(4) for r in ("true", "false")}  # <GEOM, RECORDS> -> GEOM


def _kres(kernel: str, variants: list) -> dict:
    """{template arguments as written: resources} of `kernel`'s instantiations among `variants`."""
    return {m.group(1): r for name, r in kres(kernel).items()
            if (m := re.fullmatch(rf"void trt::{kernel}<([^>]*)>\(trt::KArgs.*\)", name)) and (variants is None or m.group(1) in variants)}


@pytest.fixture(scope="module")
def resources():
    if not OBJ.exists():
        pytest.skip("build/csrc/trt_kernel.o not built")
    mine = _kres("all_hits_kernel", None)
    assert sorted(mine) == sorted(VARIANTS), mine  # exactly these
    yard = _kres("ray_query_kernel", [f"0, false, {g}, false" for g in range(4)])
    assert len(yard) == 4, yard
    return mine, {g: yard[f"0, false, {g}, false"] for g in range(4)}


def _define(src: str, name: str) -> int:
    m = re.search(rf"#define {name} (\d+)\b", src)
    assert m, name
    return int(m.group(1))


def vgpr_cap(geom: int) -> int:
    """The VGPRs a wave may hold at waves_per_simd<GEOM>() waves per SIMD (CAP = 99): 512 per SIMD
    lane, allocated in blocks of 8."""
    src = KERNEL_SRC.read_text()
    assert "__launch_bounds__(64, waves_per_simd<GEOM>()) void all_hits_kernel(" in src
    assert "return GEOM == 3 ? (CAP <= 3 ? TRT_G3_WAVES_SHALLOW : TRT_G3_WAVES) : GEOM == 0 ? TRT_G0_WAVES : TRT_WAVES;" in src
    waves = _define(src, "TRT_G3_WAVES" if geom == 3 else "TRT_G0_WAVES" if geom == 0 else "TRT_WAVES")
    assert 1 <= waves <= 8
    return (512 // waves) // 8 * 8


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_budget_against_the_hits_only_ray_query(resources, variant):
    mine, yard = resources
    geom = VARIANTS[variant]
    r, y = mine[variant], yard[geom]
    print(f"<{variant}>: all_hits_kernel {r}, ray_query_kernel<0, false, {geom}, false> {y}, VGPR cap {vgpr_cap(geom)}")
    assert r["vgpr"] <= vgpr_cap(geom), (r, vgpr_cap(geom))
    assert r["spill"] == 0, r
    assert r["lds"] <= y["lds"], (r, y)
    assert r["scratch"] <= y["scratch"], (r, y)  # the stack's private tail and nothing else


def test_triangle_free_kernels_have_no_scratch(resources):
    for v in ("0, true", "0, false"):
        assert resources[0][v]["scratch"] == 0, resources[0][v]
