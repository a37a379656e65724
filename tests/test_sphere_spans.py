"""Sphere intervals on the host (csrc/sky_spans.cpp through trt_diag_sphere_spans, no GPU): per
tile row of a launch, the tile columns [s0, s1) outside which no primary ray of any frame of the
group passes sphere_hit for any sphere.  A tile inside the row's span and outside the interval is
of the floor class (sky_trace_kernel_floor shades it without the sphere tests), so the interval
must be conservative; it must lie inside the span, be full where the span is and empty with the
spheres off; the class must be large enough on the bench's walk to be worth having; and the span
words themselves must be what they were before the intervals were added."""
from __future__ import annotations

import itertools
from pathlib import Path

import numpy as np
import pytest

from tests.floor_class_common import assert_inside_interval as _assert_inside, floor_share, intervals, raw_words
from tests.floor_class_common import sphere_hits as _sphere_hits
from tests.sky_spans_common import ADVERSARIAL, MUST_BE_FULL, NON_FINITE, ubos_at
from vkcomputeshader_tinyraytracer_amd import scene as S, types as T

ENV = (64, 32)
GOLDEN = Path(__file__).resolve().parent / "golden" / "sky_spans_parent.npz"


def _scene(w, h):
    return S.config_c2(w, h, env_size=ENV)


def _full(a, width):
    return bool((a[..., 0] == 0).all() and (a[..., 1] == (width + 7) // 8).all())


@pytest.mark.parametrize("w,h", [(128, 96), (100, 52)])
@pytest.mark.parametrize("group", [0, 2])
def test_conservative_small(w, h, group):
    """The 6-frame walk at speed 0.5 as one group and as pairs: silhouettes cross tiles."""
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 6, 0.5)
    span, sph = intervals(sc.params(), ubos, group)
    assert floor_share(span, sph, w) > 0.05
    for k in range(6):
        hits = _sphere_hits(sc, ubos[k])
        assert hits.any() and not hits.all()
        _assert_inside(hits, sph[k])


@pytest.mark.parametrize("group", [0, 16])
def test_conservative_fullres(group):
    """1024x768 over the bench's 64-position walk, positions 0, 32 and 63."""
    sc = _scene(1024, 768)
    ubos = S.camera_path(sc.ubo, 64)
    span, sph = intervals(sc.params(), ubos, group)
    for k in (0, 32, 63):
        _assert_inside(_sphere_hits(sc, ubos[k]), sph[k])


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
            span, sph = intervals(p, ubos, 0)
            assert sph.shape[1] == (len(rows) + 7) // 8
            for k in (0, 5):
                _assert_inside(_sphere_hits(sc, ubos[k]), sph[k], rows)
    assert intervals(sc.params(band_rows=4, band_count=2, band_index=1), ubos, 0) is None  # spans off: no class


@pytest.mark.parametrize("name", sorted(ADVERSARIAL))
def test_adversarial_cameras(name):
    w, h = 128, 96
    sc = _scene(w, h)
    ubos = ubos_at(sc.ubo, ADVERSARIAL[name])
    span, sph = intervals(sc.params(), ubos, 0)
    if name in MUST_BE_FULL:  # the construction's fallbacks: full rows, both
        assert _full(span, w) and _full(sph, w)
    for k in range(len(ubos)):
        _assert_inside(_sphere_hits(sc, ubos[k]), sph[k])


@pytest.mark.parametrize("cam", NON_FINITE)
def test_non_finite_cameras(cam):
    w, h = 128, 96
    sc = _scene(w, h)
    span, sph = intervals(sc.params(), ubos_at(sc.ubo, [(0.0, 0.0, 0.0), cam]), 0)
    assert _full(span, w) and _full(sph, w)
    for bad in (np.nan, np.inf):
        u = ubos_at(sc.ubo, [(0.0, 0.0, 0.0)])
        u[0]["sphere2"]["center_radius"][3] = bad
        span, sph = intervals(sc.params(), u, 0)
        assert _full(span, w) and _full(sph, w)
    assert intervals(sc.params(), ubos_at(sc.ubo, [(0.0, 0.0, 0.0)]), 0, rays_in=True) is None


@pytest.mark.parametrize("floor,spheres,quirk", list(itertools.product([False, True], repeat=3)))
def test_flag_combinations(floor, spheres, quirk):
    w, h = 128, 96
    sc = _scene(w, h)
    ubos = S.camera_path(sc.ubo, 6, 0.5)
    fl = sc.flags & ~(T.FLAG_FLOOR | T.FLAG_SPHERES | T.FLAG_ROW_QUIRK)
    fl |= (T.FLAG_FLOOR if floor else 0) | (T.FLAG_SPHERES if spheres else 0) | (T.FLAG_ROW_QUIRK if quirk else 0)
    span, sph = intervals(sc.params(flags=fl), ubos, 0)
    if not spheres:
        assert (sph[..., 0] == sph[..., 1]).all()
    if not floor:
        assert np.array_equal(span, sph)  # nothing but the balls in the span
    for k in (0, 5):
        _assert_inside(_sphere_hits(sc, ubos[k], fl), sph[k])


def test_share():
    """The bench's walk (speed 0.02) at 1024x768, a table per 16 frames.  The float64 reference
    computation of the class gives 31.8 % of a 20-frame launch's tile-frames and 31.0 % of a
    64-frame launch's."""
    sc = _scene(1024, 768)
    ubos = S.camera_path(sc.ubo, 64)
    p = sc.params()
    for n in (20, 64):
        span, sph = intervals(p, ubos[:n], 16)
        share = floor_share(span, sph, 1024)
        print(f"{n} frames: floor class {100 * share:.1f} % of tile-frames")
        assert share >= 0.28


def golden_cases():
    """name -> (params, ubos, frames per table) of the launches whose span words are recorded."""
    cases = {}
    for w, h in ((128, 96), (100, 52)):
        sc = _scene(w, h)
        ubos = S.camera_path(sc.ubo, 6, 0.5)
        for g in (0, 2):
            cases[f"walk_{w}x{h}_g{g}"] = (sc.params(), ubos, g)
        fl = sc.flags
        for name, f in (("nofloor", fl & ~T.FLAG_FLOOR), ("nospheres", fl & ~T.FLAG_SPHERES), ("noquirk", fl & ~T.FLAG_ROW_QUIRK)):
            cases[f"{name}_{w}x{h}"] = (sc.params(flags=f), ubos, 0)
    sc = _scene(100, 52)
    ubos = S.camera_path(sc.ubo, 6, 0.5)
    for count in (2, 3):
        for index in range(count):
            cases[f"band_{count}_{index}"] = (sc.params(band_rows=8, band_count=count, band_index=index), ubos, 0)
    sc = _scene(128, 96)
    for name in sorted(ADVERSARIAL):
        cases[f"adv_{name}"] = (sc.params(), ubos_at(sc.ubo, ADVERSARIAL[name]), 0)
    sc = _scene(1024, 768)
    ubos = S.camera_path(sc.ubo, 64)
    for n, g in ((20, 16), (64, 16), (64, 0)):
        cases[f"bench_{n}_g{g}"] = (sc.params(), ubos[:n], g)
    return cases


def test_spans_unchanged():
    """trt_diag_sky_spans returns the words recorded from the build before the sphere intervals."""
    gold = np.load(GOLDEN)
    cases = golden_cases()
    assert sorted(gold.files) == sorted(cases)
    for name, (p, ubos, g) in cases.items():
        tabs, shift, w = raw_words("trt_diag_sky_spans", p, ubos, g)
        rec = gold[name]  # (tables, shift) then the words
        assert (tabs, shift) == (int(rec[0]), int(rec[1])), name
        assert np.array_equal(w.reshape(-1), rec[2:]), name
