"""Lit floor on the host (no GPU): the conditions under which a floor-class launch runs
sky_trace_kernel_floor_lit (csrc/trt_runtime.cpp attach_floor_class, through trt_diag_floor_lit),
and how often its wave-uniform shortcut applies on the bench's walk.  A floor-class wave shades
without the shadow set-up when no lane that hits the floor has a bit in its shadow-mask cell; the
library's own masks (trt_diag_shadow_mask) and intervals (trt_diag_sky_spans,
trt_diag_sphere_spans) must leave at least half of the floor-class tile-frames of C2 at 1024x768
that way, or the shortcut would be vacuous."""
from __future__ import annotations

from tests.floor_class_common import intervals
from tests.floor_lit_common import class_tiles, floor_lit, scene_cells
from tests.shadow_mask_common import REF_LIGHTS
from vkcomputeshader_tinyraytracer_amd import scene as S, types as T


def test_flag_conditions():
    c2 = S.config_c2(128, 96, env_size=(64, 32))
    assert not (c2.flags & T.FLAG_CHECKER)
    assert floor_lit(c2.flags, REF_LIGHTS) == 1
    assert floor_lit(c2.flags | T.FLAG_SRGB_OUT, REF_LIGHTS) == 1
    assert floor_lit(c2.flags | T.FLAG_CHECKER, REF_LIGHTS) == 0
    assert floor_lit(S.config_c1(128, 96).flags, REF_LIGHTS) == 0
    for i in range(3):
        for y, want in [(-4.0 + 5e-3, 0), (-4.0, 0), (-10.0, 0), (float("nan"), 0), (-4.0 + 2e-2, 1)]:
            lts = REF_LIGHTS.copy()
            lts[i, 1] = y
            assert floor_lit(c2.flags, lts) == want, (i, y)


def test_lit_share_of_the_bench_walk():
    sc = S.config_c2(1024, 768, env_size=(64, 32))
    p = sc.params()
    ubos = S.camera_path(sc.ubo, 64)  # bench.py: one launch of the walk
    assert floor_lit(p.flags, REF_LIGHTS) == 1
    cells = scene_cells(sc.ubo, p.flags)
    span, sph = intervals(p, ubos)
    total = lit = hits = 0
    for f in range(0, 64, 4):
        cls, hit, dark = class_tiles(p, ubos[f], span[f], sph[f], cells)
        total += int(cls.sum())
        hits += int((cls & hit).sum())
        lit += int((cls & ~dark).sum())
    assert total > 0 and hits > 0
    share = lit / total
    print(f"floor-class tile-frames {total}, with a floor hit {hits}, without a mask bit in a floor lane {lit} "
          f"({100 * share:.1f} %)")
    assert share >= 0.5, share
