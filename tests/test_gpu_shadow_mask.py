"""Shadow occluder masks (KArgs::smask): a shadow query skips the test of a sphere that the
launch's masks prove it cannot hit.  The masks must be invisible: every frame is byte-equal to
the same frame of a context created under TRT_SHADOW_MASK=0 (sky_trace_kernel, which tests every
sphere) and of one under TRT_SKY_TABLE=0 (trace_kernel, the same), through every way a frame is
launched.  Run with `pytest -m gpu`."""
from __future__ import annotations

import numpy as np
import pytest

from tests.shadow_mask_common import (REF_LIGHTS, REF_SPHERES, cutting_floor_scene, masks, overlapping_scene,
                                      seeded_scene, ubo_with)
from vkcomputeshader_tinyraytracer_amd import Renderer, scene as S, types as T

pytestmark = pytest.mark.gpu

ENV = (64, 32)
SPEED = 0.5  # per frame: shadow outlines cross 8x8 tiles between the two frames of a pair
SIZES = [(128, 96), (100, 52)]


def _scene(w, h):
    return S.config_c2(w, h, env_size=ENV)


@pytest.fixture(scope="module")
def trio(gpu_renderer):
    """(masks on, TRT_SHADOW_MASK=0, TRT_SKY_TABLE=0): the knobs are read when a context is created."""
    made = []
    try:
        with pytest.MonkeyPatch.context() as mp:
            for k in ("TRT_SKY_TABLE", "TRT_SKY_SPANS", "TRT_SKY_SPAN_FRAMES", "TRT_SHADOW_MASK", "TRT_SHADOW_MASK_CELL"):
                mp.delenv(k, raising=False)
            made.append(Renderer(gpu_renderer.device))
            mp.setenv("TRT_SHADOW_MASK", "0")
            made.append(Renderer(gpu_renderer.device))
            mp.delenv("TRT_SHADOW_MASK")
            mp.setenv("TRT_SKY_TABLE", "0")
            made.append(Renderer(gpu_renderer.device))
        yield tuple(made)
    finally:
        for r in made:
            r.close()


def _frames(r, p, ubos, batch=0, in_flight=0):
    import torch

    n = len(ubos)
    rows = len(T.output_rows(p.height, p.band_rows, p.band_count, p.band_index))
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


def _upload(trio, sc):
    for r in trio:
        r.upload_scene(sc)


def _same_frames(trio, p, ubos, **kw):
    a = _frames(trio[0], p, ubos, **kw)
    assert np.array_equal(a, _frames(trio[1], p, ubos, **kw)), "differs from TRT_SHADOW_MASK=0"
    assert np.array_equal(a, _frames(trio[2], p, ubos, **kw)), "differs from TRT_SKY_TABLE=0"
    return a


def _same_single(trio, p, ubo):
    a = _single(trio[0], p, ubo)
    assert np.array_equal(a, _single(trio[1], p, ubo)), "differs from TRT_SHADOW_MASK=0"
    assert np.array_equal(a, _single(trio[2], p, ubo)), "differs from TRT_SKY_TABLE=0"
    return a


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("n,batch,in_flight", [(1, 0, 1), (2, 0, 1), (5, 0, 1), (5, 1, 2), (20, 0, 1), (20, 1, 2)])
def test_walk(trio, w, h, n, batch, in_flight):
    """render_frames of 1, 2, 5 and 20 frames (frame pairs, single-frame launches, two slots), and
    the same frames through draw_frame."""
    sc = _scene(w, h)
    assert not masks(REF_SPHERES, REF_LIGHTS)[2]  # this scene's masks do skip tests
    ubos = S.camera_path(sc.ubo, n, SPEED)
    p = sc.params()
    _upload(trio, sc)
    a = _same_frames(trio, p, ubos, batch=batch, in_flight=in_flight)
    for k in sorted({0, n // 2, n - 1}):
        assert np.array_equal(a[k], _same_single(trio, p, ubos[k])), k
    if n > 1:
        assert not np.array_equal(a[0], a[n - 1])


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_depths(trio, w, h, depth):
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 4, SPEED)
    _upload(trio, sc)
    _same_frames(trio, sc.params(max_depth=depth), ubos)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("flags", [
    T.FLAG_SPHERES | T.FLAG_FLOOR | T.FLAG_CHECKER | T.FLAG_ROW_QUIRK,  # C1: checker floor, constant background
    T.FLAG_SPHERES | T.FLAG_ENVMAP | T.FLAG_ROW_QUIRK,                  # floor off
    T.FLAG_FLOOR | T.FLAG_ENVMAP | T.FLAG_ROW_QUIRK,                    # spheres off: no masks
])
def test_flag_variants(trio, w, h, flags):
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 4, SPEED)
    _upload(trio, sc)
    for depth in (1, 4):
        p = sc.params(max_depth=depth)
        p.flags = flags
        a = _same_frames(trio, p, ubos)
        assert np.array_equal(a[1], _same_single(trio, p, ubos[1]))


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("count", [2, 3])
def test_bands(trio, w, h, count):
    """Band launches of 8 rows against the rows of the full frames."""
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 4, SPEED)
    _upload(trio, sc)
    full = _frames(trio[2], sc.params(), ubos)
    for index in range(count):
        p = sc.params(band_rows=8, band_count=count, band_index=index)
        a = _same_frames(trio, p, ubos)
        assert np.array_equal(a, full[:, T.output_rows(h, 8, count, index)])


@pytest.mark.parametrize("w,h", SIZES)
def test_scene_changes_between_launches(trio, w, h):
    """The masks follow the UBO: spheres and lights change between launches on one context, inside
    one render_frames call and between calls (key change, then rebuild), and back."""
    sc = _scene(w, h)
    p = sc.params()
    _upload(trio, sc)
    base = S.camera_path(sc.ubo, 4, SPEED)
    first = _same_frames(trio, p, base)
    variants = [seeded_scene(1), cutting_floor_scene(), overlapping_scene(), seeded_scene(3)]
    for sph, lts in variants:
        assert not masks(sph, lts)[2]
        moved = np.array([ubo_with(u, sph, lts) for u in base])
        second = _same_frames(trio, p, moved)
        assert not np.array_equal(first, second)
        assert np.array_equal(second[2], _same_single(trio, p, moved[2]))
    # one call whose launches alternate between two scenes: a rebuild per launch
    sph, lts = seeded_scene(2)
    mixed = base.copy()
    for k in (1, 3):
        mixed[k] = ubo_with(base[k], sph, lts)
    a = _same_frames(trio, p, mixed)
    assert np.array_equal(a[0], first[0]) and np.array_equal(a[2], first[2])
    assert np.array_equal(_same_frames(trio, p, base), first)  # and back


@pytest.mark.parametrize("w,h", SIZES)
def test_fallback_scenes(trio, w, h):
    """Scenes whose masks are all ones: a light inside a sphere, a light on the floor plane, a
    non-finite sphere; and a camera outside the construction's error bound."""
    sc = _scene(w, h)
    p = sc.params()
    _upload(trio, sc)
    base = S.camera_path(sc.ubo, 4, SPEED)
    inside = REF_LIGHTS.copy()
    inside[1] = (7.0, 5.0, -15.0)
    on_floor = REF_LIGHTS.copy()
    on_floor[0] = (-20.0, -4.0, 20.0)
    nan_sphere = REF_SPHERES.copy()
    nan_sphere[2, 0] = np.nan
    for sph, lts in [(REF_SPHERES, inside), (REF_SPHERES, on_floor), (nan_sphere, REF_LIGHTS)]:
        assert masks(sph, lts)[2]
        _same_frames(trio, p, np.array([ubo_with(u, sph, lts) for u in base]))
    far = base.copy()
    far[1]["camPos"][:3] = (0.0, 30.0, 200.0)
    far[2]["camPos"][:3] = (np.nan, 0.0, 0.0)
    a = _same_frames(trio, p, far)
    assert np.array_equal(a[1], _same_single(trio, p, far[1]))
