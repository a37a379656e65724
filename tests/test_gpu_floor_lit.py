"""Lit floor (sky_trace_kernel_floor_lit): a floor-class launch whose floor is grey
and whose lights all lie above the floor plane carries the floor's colour as one channel, and a wave
none of whose floor lanes has a shadow-mask bit shades without the shadow set-up.  Both must be
invisible: every frame is byte-equal to the same frame of contexts created under TRT_FLOOR_LIT=0
(sky_trace_kernel_floor), TRT_FLOOR_CLASS=0 (sky_trace_kernel_smask) and TRT_SKY_TABLE=0
(trace_kernel).  Run with `pytest -m gpu`."""
from __future__ import annotations

import numpy as np
import pytest

from tests.floor_class_common import intervals
from tests.floor_lit_common import class_tiles, floor_lit, scene_cells, tiles
from tests.shadow_mask_common import REF_LIGHTS, ubo_with
from tests.sky_spans_common import hits
from vkcomputeshader_tinyraytracer_amd import Renderer, scene as S, types as T

pytestmark = pytest.mark.gpu

ENV = (64, 32)
SPEED = 0.5  # per frame: the horizon, the floor's edges and the shadow outlines cross 8x8 tiles within a pair
SIZES = [(128, 96), (100, 52)]
KNOBS = ("TRT_SKY_TABLE", "TRT_SKY_SPANS", "TRT_SKY_SPAN_FRAMES", "TRT_SHADOW_MASK", "TRT_SHADOW_MASK_CELL",
         "TRT_FLOOR_CLASS", "TRT_FLOOR_LIT")
OFF = ("TRT_FLOOR_LIT", "TRT_FLOOR_CLASS", "TRT_SKY_TABLE")
# light 0 low in the west: the spheres' shadows run far across the floor-class tiles
LOW_LIGHT = np.array([(-20.0, 6.0, -10.0), REF_LIGHTS[1], REF_LIGHTS[2]], np.float32)


@pytest.fixture(scope="module")
def quad(gpu_renderer):
    """(default, TRT_FLOOR_LIT=0, TRT_FLOOR_CLASS=0, TRT_SKY_TABLE=0): the knobs are read when a
    context is created."""
    made = []
    try:
        with pytest.MonkeyPatch.context() as mp:
            for k in KNOBS:
                mp.delenv(k, raising=False)
            made.append(Renderer(gpu_renderer.device))
            for knob in OFF:
                mp.setenv(knob, "0")
                made.append(Renderer(gpu_renderer.device))
                mp.delenv(knob)
        yield tuple(made)
    finally:
        for r in made:
            r.close()


def _frames(r, p, ubos, in_place_rows=None):
    import torch

    n = len(ubos)
    rows = in_place_rows if in_place_rows is not None else len(
        T.output_rows(p.height, p.band_rows, p.band_count, p.band_index))
    out = torch.zeros((n, rows, p.width, 4), dtype=torch.uint8, device=f"cuda:{r.device}")
    torch.cuda.synchronize(r.device)  # the fill runs on torch's stream, the frames on the context's
    r.set_frame_batch(0)  # one multi-frame launch (at most 6 frames here)
    r.set_frames_in_flight(1)
    try:
        r.render_frames(p, out, n, ubos=ubos, frame_stride=rows * p.width * 4)
        r.synchronize()
    finally:
        r.set_frames_in_flight(0)
    return out.cpu().numpy()


def _same_frames(quad, sc, p, ubos, **kw):
    for r in quad:
        r.upload_scene(sc)
    a = _frames(quad[0], p, ubos, **kw)
    for r, knob in zip(quad[1:], OFF):
        assert np.array_equal(a, _frames(r, p, ubos, **kw)), f"differs from {knob}=0"
    return a


def _lights(ubo):
    return np.array([ubo[f"light{i}"][:3] for i in range(3)], np.float32)


def _waves(p, ubos):
    """(floor-class tile-frames with a floor hit and no mask bit, with a mask bit) of a launch of
    full frames, by the host model."""
    cells = scene_cells(ubos[0], p.flags)
    span, sph = intervals(p, ubos)
    lit = dark = 0
    for f in range(len(ubos)):
        cls, hit, drk = class_tiles(p, ubos[f], span[f], sph[f], cells)
        lit += int((cls & hit & ~drk).sum())
        dark += int((cls & drk).sum())
    return lit, dark


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("n", [6, 5])
def test_walk(quad, w, h, n):
    """One launch of 6 frames, and of 5, whose last pair holds one frame."""
    sc = S.config_c2(w, h, env_size=ENV)
    ubos = S.camera_path(sc.ubo, n, SPEED)
    p = sc.params()
    assert floor_lit(p.flags, _lights(ubos[0])) == 1
    lit, _ = _waves(p, ubos)
    assert lit > 0
    a = _same_frames(quad, sc, p, ubos)
    assert not np.array_equal(a[0], a[n - 1])


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("count", [2, 3])
@pytest.mark.parametrize("in_place", [False, True])
def test_bands(quad, w, h, count, in_place):
    """Band launches of 8 rows, compact and in place, against the rows of the full frames."""
    sc = S.config_c2(w, h, env_size=ENV)
    ubos = S.camera_path(sc.ubo, 6, SPEED)
    for r in quad:
        r.upload_scene(sc)
    full = _frames(quad[3], sc.params(), ubos)
    for index in range(count):
        p = sc.params(band_rows=8, band_count=count, band_index=index)
        if in_place:
            p.flags |= T.FLAG_BAND_IN_PLACE
        rows = T.output_rows(h, 8, count, index)
        a = _same_frames(quad, sc, p, ubos, in_place_rows=h if in_place else None)
        assert np.array_equal(a[:, rows] if in_place else a, full[:, rows])


@pytest.mark.parametrize("w,h", SIZES)
def test_checker_floor(quad, w, h):
    """C1, and C2 with the checker: the flag is off, the frames still equal."""
    for sc, fl in [(S.config_c1(w, h), None), (S.config_c2(w, h, env_size=ENV), T.FLAG_CHECKER)]:
        p = sc.params() if fl is None else sc.params(flags=sc.flags | fl)
        ubos = S.camera_path(sc.ubo, 6, SPEED)
        assert floor_lit(p.flags, _lights(ubos[0])) == 0
        _same_frames(quad, sc, p, ubos)


@pytest.mark.parametrize("w,h", SIZES)
def test_light_below_the_floor(quad, w, h):
    """One light at y = -10: the flag is off (the floor's underside faces it)."""
    sc = S.config_c2(w, h, env_size=ENV)
    p = sc.params()
    base = S.camera_path(sc.ubo, 6, SPEED)
    ref = _same_frames(quad, sc, p, base)
    for i in range(3):
        lts = REF_LIGHTS.copy()
        lts[i, 1] = -10.0
        assert floor_lit(p.flags, lts) == 0
        ubos = np.array([ubo_with(u, None, lts) for u in base])
        a = _same_frames(quad, sc, p, ubos)
        assert not np.array_equal(a, ref)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("srgb", [False, True])
def test_shadows_across_the_class(quad, w, h, srgb):
    """A low light: waves with and without a mask bit in one frame, linear and sRGB bytes."""
    sc = S.config_c2(w, h, env_size=ENV)
    p = sc.params(flags=sc.flags | (T.FLAG_SRGB_OUT if srgb else 0))
    ubos = np.array([ubo_with(u, None, LOW_LIGHT) for u in S.camera_path(sc.ubo, 6, SPEED)])
    assert floor_lit(p.flags, LOW_LIGHT) == 1
    lit, dark = _waves(p, ubos)
    assert lit > 0 and dark > 0
    _same_frames(quad, sc, p, ubos)


@pytest.mark.parametrize("w,h", SIZES)
def test_srgb_out(quad, w, h):
    sc = S.config_c2(w, h, env_size=ENV)
    ubos = S.camera_path(sc.ubo, 6, SPEED)
    a = _same_frames(quad, sc, sc.params(flags=sc.flags | T.FLAG_SRGB_OUT), ubos)
    assert not np.array_equal(a, _frames(quad[0], sc.params(), ubos))


def test_floor_edge_inside_a_lit_wave():
    """At 128x96 a floor-class tile holds floor hits and primary misses (the oracle's depth-1 hit
    mask): lanes that store their sky word inside a wave that shades the floor (test_walk)."""
    w, h = SIZES[0]
    sc = S.config_c2(w, h, env_size=ENV)
    p = sc.params()
    ubos = S.camera_path(sc.ubo, 6, SPEED)
    cells = scene_cells(ubos[0], p.flags)
    span, sph = intervals(p, ubos)
    mixed = 0
    for f in range(len(ubos)):
        cls, _, dark = class_tiles(p, ubos[f], span[f], sph[f], cells)
        m = hits(sc, ubos[f])
        mixed += int((cls & ~dark & tiles(m) & tiles(~m)).sum())
    assert mixed > 0
