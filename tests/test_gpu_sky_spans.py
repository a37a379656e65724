"""Sky spans (KArgs::span): a tile outside its row's span stores its sky-table words without
generating or intersecting its primary rays.  The spans must be invisible: every frame is
byte-equal to the same frame of a context created under TRT_SKY_SPANS=0 (the sky table's own
test per tile) and of one under TRT_SKY_TABLE=0 (the per-ray background), through every way a
frame is launched.  Run with `pytest -m gpu`."""
from __future__ import annotations

import numpy as np
import pytest

from tests.sky_spans_common import ADVERSARIAL, NON_FINITE, culled_share, is_full, spans, ubos_at
from vkcomputeshader_tinyraytracer_amd import Renderer, scene as S, types as T

pytestmark = pytest.mark.gpu

ENV = (64, 32)
SPEED = 0.5  # per frame: silhouettes cross 8x8 tiles between the two frames of a pair
SIZES = [(128, 96), (100, 52)]


def _scene(w, h):
    return S.config_c2(w, h, env_size=ENV)


@pytest.fixture(scope="module")
def trio(gpu_renderer):
    """(spans on, TRT_SKY_SPANS=0, TRT_SKY_TABLE=0): the knobs are read when a context is created."""
    made = []
    try:
        with pytest.MonkeyPatch.context() as mp:
            mp.delenv("TRT_SKY_TABLE", raising=False)
            mp.delenv("TRT_SKY_SPANS", raising=False)
            mp.delenv("TRT_SKY_SPAN_FRAMES", raising=False)
            made.append(Renderer(gpu_renderer.device))
            mp.setenv("TRT_SKY_SPANS", "0")
            made.append(Renderer(gpu_renderer.device))
            mp.delenv("TRT_SKY_SPANS")
            mp.setenv("TRT_SKY_TABLE", "0")
            made.append(Renderer(gpu_renderer.device))
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


def _upload(trio, sc):
    for r in trio:
        r.upload_scene(sc)


def _same_frames(trio, p, ubos, **kw):
    a = _frames(trio[0], p, ubos, **kw)
    assert np.array_equal(a, _frames(trio[1], p, ubos, **kw)), "differs from TRT_SKY_SPANS=0"
    assert np.array_equal(a, _frames(trio[2], p, ubos, **kw)), "differs from TRT_SKY_TABLE=0"
    return a


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("batch", [0, 1])
def test_walk(trio, w, h, batch, in_flight):
    """The 6-frame walk through frame pairs, single-frame launches and two slots."""
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 6, SPEED)
    p = sc.params()
    assert culled_share(spans(p, ubos), w) > 0.05  # the spans do cull tiles of this launch
    _upload(trio, sc)
    a = _same_frames(trio, p, ubos, batch=batch, in_flight=in_flight)
    for k in range(6):
        assert np.array_equal(a[k], _single(trio[0], p, ubos[k])), k
    assert not np.array_equal(a[0], a[5])


@pytest.mark.parametrize("w,h", SIZES)
def test_odd_last_pair(trio, w, h):
    """9 frames: the last frame pair has one frame."""
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 9, SPEED)
    _upload(trio, sc)
    a = _same_frames(trio, sc.params(), ubos)
    assert np.array_equal(a[8], _single(trio[2], sc.params(), ubos[8]))


@pytest.mark.parametrize("w,h", SIZES)
def test_adversarial_cameras(trio, w, h):
    """Each camera as a single draw_frame, and all of them inside one render_frames call."""
    sc = _scene(w, h)
    p = sc.params()
    _upload(trio, sc)
    cams = [c for name in sorted(ADVERSARIAL) for c in ADVERSARIAL[name]] + NON_FINITE
    ubos = ubos_at(sc.ubo, cams)
    _same_frames(trio, p, ubos)
    _same_frames(trio, p, ubos, batch=2)
    for u in ubos:
        a = _single(trio[0], p, u)
        assert np.array_equal(a, _single(trio[1], p, u)) and np.array_equal(a, _single(trio[2], p, u))


@pytest.mark.parametrize("w,h", SIZES)
def test_sphere_moved_between_calls(trio, w, h):
    """The spans follow the UBO's spheres: one moved and resized by update_ubo between calls."""
    sc = _scene(w, h)
    p = sc.params()
    _upload(trio, sc)
    ubos = S.camera_path(sc.ubo, 6, SPEED)
    first = _same_frames(trio, p, ubos)
    moved = ubos.copy()
    for u in moved:
        u["sphere3"]["center_radius"] = (-9.0, 6.0, -14.0, 1.5)
    assert not np.array_equal(spans(p, moved), spans(p, ubos))
    second = _same_frames(trio, p, moved)
    assert not np.array_equal(first, second)
    a = _single(trio[0], p, moved[3])
    assert np.array_equal(a, second[3]) and np.array_equal(a, _single(trio[2], p, moved[3]))
    assert np.array_equal(_same_frames(trio, p, ubos), first)  # and back


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("count", [2, 3])
@pytest.mark.parametrize("w,h", SIZES)
def test_bands(trio, w, h, count, in_place):
    """Band groups of 8 rows: the spans are indexed by compact tile row, the screen by frame row."""
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 6, SPEED)
    _upload(trio, sc)
    full = _frames(trio[2], sc.params(), ubos)
    for index in range(count):
        p = sc.params(band_rows=8, band_count=count, band_index=index)
        if in_place:
            p.flags |= T.FLAG_BAND_IN_PLACE
        assert not is_full(spans(p, ubos), w)
        rows = T.output_rows(h, 8, count, index)
        a = _same_frames(trio, p, ubos, in_place_rows=h if in_place else None)
        assert np.array_equal(a[:, rows] if in_place else a, full[:, rows])


@pytest.mark.parametrize("w,h", SIZES)
def test_bands_of_four_rows(trio, w, h):
    """band_rows 4: a tile row's frame rows are not consecutive, so the launch runs with spans off."""
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 6, SPEED)
    _upload(trio, sc)
    full = _frames(trio[2], sc.params(), ubos)
    for index in range(2):
        p = sc.params(band_rows=4, band_count=2, band_index=index)
        assert is_full(spans(p, ubos), w)
        a = _same_frames(trio, p, ubos)
        assert np.array_equal(a, full[:, T.output_rows(h, 4, 2, index)])
