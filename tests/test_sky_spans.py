"""Sky spans on the host (csrc/sky_spans.cpp through trt_diag_sky_spans, no GPU): per tile row of
a launch, the tile columns outside which no primary ray of any frame of the group hits the floor
or a sphere.  They must be conservative (every pixel the oracle's primary ray hits lies inside
its row's span, for every frame of the group), fall back to full rows where the construction
does not apply, and cull enough of the bench's walk to be worth having."""
from __future__ import annotations

import numpy as np
import pytest

from tests.sky_spans_common import (ADVERSARIAL, MUST_BE_FULL, assert_inside as _assert_inside, culled_share, hits as _hits,
                                    is_full, spans, ubos_at)
from vkcomputeshader_tinyraytracer_amd import scene as S, types as T

ENV = (64, 32)


def _scene(w, h):
    return S.config_c2(w, h, env_size=ENV)


@pytest.mark.parametrize("w,h", [(128, 96), (100, 52)])
@pytest.mark.parametrize("group", [0, 2])
def test_conservative_small(w, h, group):
    """The 6-frame walk at speed 0.5 as one group and as pairs: silhouettes cross tiles."""
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 6, 0.5)
    sp = spans(sc.params(), ubos, group)
    assert not is_full(sp, w) and culled_share(sp, w) > 0.05
    for k in range(6):
        hits = _hits(sc, ubos[k])
        assert hits.any() and not hits.all()
        _assert_inside(hits, sp[k])


@pytest.mark.parametrize("group", [0, 16])
def test_conservative_fullres(group):
    """1024x768 over the bench's 64-position walk, positions 0, 32 and 63."""
    sc = _scene(1024, 768)
    ubos = S.camera_path(sc.ubo, 64)
    sp = spans(sc.params(), ubos, group)
    for k in (0, 32, 63):
        _assert_inside(_hits(sc, ubos[k]), sp[k])


@pytest.mark.parametrize("in_place", [False, True])
def test_conservative_bands(in_place):
    """Band launches index the table by compact tile row and the screen by frame row."""
    w, h = 100, 52
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 6, 0.5)
    for count in (2, 3):
        for index in range(count):
            p = sc.params(band_rows=8, band_count=count, band_index=index)
            if in_place:
                p.flags |= T.FLAG_BAND_IN_PLACE
            rows = T.output_rows(h, 8, count, index)
            sp = spans(p, ubos, 0)
            assert sp.shape[1] == (len(rows) + 7) // 8
            for k in (0, 5):
                _assert_inside(_hits(sc, ubos[k]), sp[k], rows)
    assert is_full(spans(sc.params(band_rows=4, band_count=2, band_index=1), ubos, 0), w)  # spans off


@pytest.mark.parametrize("name", sorted(ADVERSARIAL))
def test_adversarial_cameras(name):
    w, h = 128, 96
    sc = _scene(w, h)
    ubos = ubos_at(sc.ubo, ADVERSARIAL[name])
    sp = spans(sc.params(), ubos, 0)
    if name in MUST_BE_FULL:
        assert is_full(sp, w)
    if name == "scene_behind":
        assert culled_share(sp, w) == 1.0
    for k in range(len(ubos)):
        _assert_inside(_hits(sc, ubos[k]), sp[k])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_inputs(bad):
    w, h = 128, 96
    sc = _scene(w, h)
    for axis in range(3):
        cam = [0.0, 0.0, 0.0]
        cam[axis] = bad
        assert is_full(spans(sc.params(), ubos_at(sc.ubo, [(0.0, 0.0, 0.0), tuple(cam)]), 0), w)
    u = ubos_at(sc.ubo, [(0.0, 0.0, 0.0)])
    u[0]["sphere2"]["center_radius"][3] = bad
    assert is_full(spans(sc.params(), u, 0), w)
    u = ubos_at(sc.ubo, [(0.0, 0.0, 0.0)])
    u[0]["sphere0"]["center_radius"][1] = bad
    assert is_full(spans(sc.params(), u, 0), w)
    assert is_full(spans(sc.params(), ubos_at(sc.ubo, [(0.0, 0.0, 0.0)]), 0, rays_in=True), w)


def test_moved_sphere():
    """The spheres come from the UBO: one moved and resized shows in the spans."""
    w, h = 128, 96
    sc = _scene(w, h)
    u = ubos_at(sc.ubo, [(0.0, 0.0, 0.0)])
    u[0]["sphere3"]["center_radius"] = (-9.0, 6.0, -14.0, 1.5)
    sp = spans(sc.params(), u, 0)
    assert not np.array_equal(sp, spans(sc.params(), ubos_at(sc.ubo, [(0.0, 0.0, 0.0)]), 0))
    _assert_inside(_hits(sc, u[0]), sp[0])


def test_flags():
    """No floor, no spheres, neither, and C1's checker floor."""
    w, h = 128, 96
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 6, 0.5)
    base = sc.flags
    assert base & T.FLAG_FLOOR and base & T.FLAG_SPHERES
    shares = {}
    for name, fl in (("both", base), ("no_floor", base & ~T.FLAG_FLOOR), ("no_spheres", base & ~T.FLAG_SPHERES),
                     ("neither", base & ~T.FLAG_FLOOR & ~T.FLAG_SPHERES)):
        sp = spans(sc.params(flags=fl), ubos, 0)
        shares[name] = culled_share(sp, w)
        for k in (0, 5):
            _assert_inside(_hits(sc, ubos[k], fl), sp[k])
    assert shares["neither"] == 1.0
    assert shares["both"] < min(shares["no_floor"], shares["no_spheres"])
    c1 = S.config_c1(w, h)
    assert c1.flags & T.FLAG_CHECKER
    u1 = S.camera_path(c1.ubo, 6, 0.5)
    sp = spans(c1.params(), u1, 0)
    assert not is_full(sp, w)
    for k in (0, 5):
        _assert_inside(_hits(c1, u1[k], c1.flags), sp[k])


def test_not_vacuous():
    """The bench's walk (speed 0.02) at 1024x768.  The float64 prototype of the construction culls
    39.8 % of a 20-frame launch's tiles and 31.5 % of a 64-frame launch's with one table; the
    floors leave room for a looser but still rigorous chord bound."""
    sc = _scene(1024, 768)
    ubos = S.camera_path(sc.ubo, 64)
    p = sc.params()
    assert culled_share(spans(p, ubos[:20], 0), 1024) >= 0.35
    assert culled_share(spans(p, ubos[:20], 16), 1024) >= 0.35  # the default: a table per 16 frames
    assert culled_share(spans(p, ubos, 0), 1024) >= 0.27
    assert culled_share(spans(p, ubos, 16), 1024) >= 0.35
