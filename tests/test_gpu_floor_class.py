"""Floor class (KArgs::floor_class, sky_trace_kernel_floor): a tile inside its row's span and
outside its row's sphere interval skips the primary sphere tests and shades its floor hits
straight-line, once per frame pair for the direction and the sky word.  The class must be
invisible: every frame is byte-equal to the same frame of contexts created under
TRT_FLOOR_CLASS=0 (sky_trace_kernel_smask), TRT_SHADOW_MASK=0 (sky_trace_kernel) and
TRT_SKY_TABLE=0 (trace_kernel), through every way a frame is launched.  Run with `pytest -m gpu`."""
from __future__ import annotations

import numpy as np
import pytest

from tests.floor_class_common import floor_tiles, intervals
from tests.shadow_mask_common import REF_LIGHTS, REF_SPHERES, seeded_scene, ubo_with
from tests.sky_spans_common import ubos_at
from vkcomputeshader_tinyraytracer_amd import Renderer, scene as S, types as T

pytestmark = pytest.mark.gpu

ENV = (64, 32)
SPEED = 0.5  # per frame: the horizon, the floor's edges and the shadow outlines cross 8x8 tiles within a pair
SIZES = [(128, 96), (100, 52)]
KNOBS = ("TRT_SKY_TABLE", "TRT_SKY_SPANS", "TRT_SKY_SPAN_FRAMES", "TRT_SHADOW_MASK", "TRT_SHADOW_MASK_CELL",
         "TRT_FLOOR_CLASS")
NAMES = ("default", "TRT_FLOOR_CLASS=0", "TRT_SHADOW_MASK=0", "TRT_SKY_TABLE=0")


def _scene(w, h):
    return S.config_c2(w, h, env_size=ENV)


@pytest.fixture(scope="module")
def quad(gpu_renderer):
    """(default, TRT_FLOOR_CLASS=0, TRT_SHADOW_MASK=0, TRT_SKY_TABLE=0): the knobs are read when a
    context is created."""
    made = []
    try:
        with pytest.MonkeyPatch.context() as mp:
            for k in KNOBS:
                mp.delenv(k, raising=False)
            made.append(Renderer(gpu_renderer.device))
            for knob in ("TRT_FLOOR_CLASS", "TRT_SHADOW_MASK", "TRT_SKY_TABLE"):
                mp.setenv(knob, "0")
                made.append(Renderer(gpu_renderer.device))
                mp.delenv(knob)
        yield tuple(made)
    finally:
        for r in made:
            r.close()


def _frames(r, p, ubos, batch=0, in_flight=0, in_place_rows=None):
    import torch

    n = len(ubos)
    rows = in_place_rows if in_place_rows is not None else len(
        T.output_rows(p.height, p.band_rows, p.band_count, p.band_index))
    out = torch.zeros((n, rows, p.width, 4), dtype=torch.uint8, device=f"cuda:{r.device}")
    torch.cuda.synchronize(r.device)  # the fill runs on torch's stream, the frames on the context's
    r.set_frame_batch(batch)
    r.set_frames_in_flight(in_flight)
    try:
        r.render_frames(p, out, n, ubos=ubos, frame_stride=rows * p.width * 4)
        r.synchronize()
    finally:
        r.set_frame_batch(0)
        r.set_frames_in_flight(0)
    return out.cpu().numpy()


def _single(r, p, ubo):
    r.update_ubo(ubo)
    return r.draw_frame(p)[0]


def _upload(quad, sc):
    for r in quad:
        r.upload_scene(sc)


def _same_frames(quad, p, ubos, **kw):
    a = _frames(quad[0], p, ubos, **kw)
    for r, name in zip(quad[1:], NAMES[1:]):
        assert np.array_equal(a, _frames(r, p, ubos, **kw)), f"differs from {name}"
    return a


def _same_single(quad, p, ubo):
    a = _single(quad[0], p, ubo)
    for r, name in zip(quad[1:], NAMES[1:]):
        assert np.array_equal(a, _single(r, p, ubo)), f"differs from {name}"
    return a


def _class_tiles(p, ubos):
    """Floor-class tile-frames of one launch of these frames (at most 20 here, so one launch of
    batch 0 holds them all); 0 where the spans are off.  A launch of one frame (one frame given,
    batch 1, draw_frame) runs without the class, whatever its intervals say: it must only match."""
    if len(ubos) < 2:
        return 0
    iv = intervals(p, ubos)
    return floor_tiles(*iv) if iv is not None else 0


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("n,batch,in_flight", [(1, 0, 1), (2, 0, 1), (5, 0, 1), (5, 1, 2), (9, 0, 1), (20, 0, 1),
                                               (20, 1, 2), (20, 0, 2)])
def test_walk(quad, w, h, n, batch, in_flight):
    """render_frames of 1, 2, 5, 9 (an odd last pair) and 20 frames as frame pairs (with the class)
    and as single-frame launches (without), in one and two slots, and the same frames through
    draw_frame."""
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, n, SPEED)
    p = sc.params()
    if n > 1 and batch == 0:
        assert _class_tiles(p, ubos) > 0
    _upload(quad, sc)
    a = _same_frames(quad, p, ubos, batch=batch, in_flight=in_flight)
    for k in sorted({0, n // 2, n - 1}):
        assert np.array_equal(a[k], _same_single(quad, p, ubos[k])), k
    if n > 1:
        assert not np.array_equal(a[0], a[n - 1])


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_depths(quad, w, h, depth):
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 4, SPEED)
    p = sc.params(max_depth=depth)
    assert _class_tiles(p, ubos) > 0
    _upload(quad, sc)
    _same_frames(quad, p, ubos)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("checker", [False, True])
@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("quirk", [False, True])
def test_flag_variants(quad, w, h, checker, srgb, quirk):
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 4, SPEED)
    _upload(quad, sc)
    fl = (sc.flags & ~(T.FLAG_CHECKER | T.FLAG_SRGB_OUT | T.FLAG_ROW_QUIRK)) | (T.FLAG_CHECKER if checker else 0) | (
        T.FLAG_SRGB_OUT if srgb else 0) | (T.FLAG_ROW_QUIRK if quirk else 0)
    p = sc.params(flags=fl)
    assert _class_tiles(p, ubos) > 0
    a = _same_frames(quad, p, ubos)
    assert np.array_equal(a[1], _same_single(quad, p, ubos[1]))


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("off", [T.FLAG_SPHERES, T.FLAG_FLOOR, T.FLAG_SPHERES | T.FLAG_FLOOR])
def test_scene_parts_off(quad, w, h, off):
    """Spheres off, floor off, both: launches without the class (today's kernels) still match."""
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 4, SPEED)
    _upload(quad, sc)
    for depth in (1, 4):
        p = sc.params(max_depth=depth, flags=sc.flags & ~off)
        a = _same_frames(quad, p, ubos)
        assert np.array_equal(a[1], _same_single(quad, p, ubos[1]))


@pytest.mark.parametrize("w,h", SIZES)
def test_scene_changes_between_calls(quad, w, h):
    """A sphere moved, then a light moved, between calls on one context, and back."""
    sc = _scene(w, h)
    p = sc.params()
    _upload(quad, sc)
    base = S.camera_path(sc.ubo, 4, SPEED)
    first = _same_frames(quad, p, base)
    sph = REF_SPHERES.copy()
    sph[3] = (-6.0, 3.0, -14.0, 1.5)
    lts = REF_LIGHTS.copy()
    lts[0] = (25.0, 30.0, 10.0)
    prev = first
    for s, l in [(sph, None), (sph, lts), seeded_scene(1)]:
        moved = np.array([ubo_with(u, s, l) for u in base])
        assert _class_tiles(p, moved) > 0
        cur = _same_frames(quad, p, moved)
        assert not np.array_equal(prev, cur)
        assert np.array_equal(cur[2], _same_single(quad, p, moved[2]))
        prev = cur
    assert np.array_equal(_same_frames(quad, p, base), first)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("count", [2, 3])
@pytest.mark.parametrize("in_place", [False, True])
def test_bands(quad, w, h, count, in_place):
    """Band launches of 8 rows, compact and in place, against the rows of the full frames."""
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 4, SPEED)
    _upload(quad, sc)
    full = _frames(quad[3], sc.params(), ubos)
    tiles = 0
    for index in range(count):
        p = sc.params(band_rows=8, band_count=count, band_index=index)
        if in_place:
            p.flags |= T.FLAG_BAND_IN_PLACE
        tiles += _class_tiles(p, ubos)
        rows = T.output_rows(h, 8, count, index)
        a = _same_frames(quad, p, ubos, in_place_rows=h if in_place else None)
        assert np.array_equal(a[:, rows] if in_place else a, full[:, rows])
    assert tiles > 0


@pytest.mark.parametrize("w,h", SIZES)
def test_bands_of_four_rows(quad, w, h):
    """band_rows 4: the launch runs with spans off, so without the class."""
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 4, SPEED)
    _upload(quad, sc)
    full = _frames(quad[3], sc.params(), ubos)
    for index in range(2):
        p = sc.params(band_rows=4, band_count=2, band_index=index)
        assert _class_tiles(p, ubos) == 0
        a = _same_frames(quad, p, ubos)
        assert np.array_equal(a, full[:, T.output_rows(h, 4, 2, index)])


@pytest.mark.parametrize("w,h", SIZES)
def test_low_and_high_cameras(quad, w, h):
    """A camera low above the floor beside the spheres (floor from the bottom edge to the horizon,
    most hit tiles of the class) and one so high that no pixel hits the floor."""
    sc = _scene(w, h)
    p = sc.params()
    _upload(quad, sc)
    low = ubos_at(sc.ubo, [(6.0 + 0.1 * k, -2.0, -4.0 - 0.1 * k) for k in range(4)])
    assert _class_tiles(p, low) > 0
    a = _same_frames(quad, p, low)
    assert np.array_equal(a[3], _same_single(quad, p, low[3]))
    high = ubos_at(sc.ubo, [(0.0, 40.0 + 0.5 * k, 0.0) for k in range(4)])
    b = _same_frames(quad, p, high)
    assert np.array_equal(b[0], _same_single(quad, p, high[0]))
    assert not np.array_equal(a[0], b[0])
