"""The scenes of tests/random_scenes.py on the CPU: the oracle is a usable referee on them (its
literal and fast restatements agree bit for bit and every colour is finite), the host proofs the
fast C2 paths rest on hold on their geometry (sky spans, sphere intervals, shadow occluder masks),
and the set is not vacuous (spans that cull, floor-class tiles, masks without the fallback, rays of
every kind).  tests/test_gpu_random_scenes.py renders the same scenes on the GPU."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as orc
from tests import random_scenes as R
from tests.floor_class_common import assert_inside_interval, floor_tiles, intervals, sphere_hits
from tests.shadow_mask_common import F, bits, cell_masks, dot, floor_points, masks, query_needs
from tests.sky_spans_common import assert_inside, hits, is_full, spans
from vkcomputeshader_tinyraytracer_amd import scene as S

ALL = R.all_cases()
N_FLOOR = 24_000  # shadow queries sampled per scene: floor points, and points per sphere
N_SPHERE = 4_000
_STATS: dict = {}


def _depths(name):
    return (R.seed_depth(int(name[4:])),) if name.startswith("seed") else R.CASE_DEPTHS


def _walk(case):
    """The 4-frame launch of the host-proof checks, with the reference materials (hit masks come
    from colour != background)."""
    return S.camera_path(case.with_reference_materials(), 4, R.WALK_SPEED)


@pytest.mark.parametrize("name", sorted(ALL))
def test_oracle_modes_agree_and_are_finite(name):
    case = ALL[name]
    sc = case.scene()
    for depth in _depths(name):
        p = case.params(max_depth=depth)
        a8, a32, ast = orc.render(sc, p, mode=orc.MODE_FAST, want32=True)
        b8, b32, bst = orc.render(sc, p, mode=orc.MODE_LITERAL, want32=True)
        assert np.isfinite(a32).all() and np.isfinite(b32).all(), depth
        assert np.array_equal(a8, b8), depth
        assert np.array_equal(a32.view(np.uint32), b32.view(np.uint32)), depth
        assert ast == bst, depth
        assert ast["primary_rays"] == case.width * case.height
        _STATS[name, depth] = ast


@pytest.mark.parametrize("name", sorted(ALL))
def test_spans_and_intervals_hold_every_primary_hit(name):
    case = ALL[name]
    ubos = _walk(case)
    p = case.params()
    sp = spans(p, ubos)
    iv = intervals(p, ubos)
    for k in range(len(ubos)):
        sc = case.scene(ubos[k])
        assert_inside(hits(sc, ubos[k], fov=case.fov), sp[k])
        if iv is not None:
            assert np.array_equal(iv[0][k], sp[k])
            assert_inside_interval(sphere_hits(sc, ubos[k], fov=case.fov), iv[1][k])


@pytest.mark.parametrize("name", sorted(ALL))
def test_shadow_masks_keep_every_needed_bit(name):
    case = ALL[name]
    sph, lts = case.geometry()
    cells, rows, _ = masks(sph, lts, flags=case.flags)
    cell = 0.25
    p, _ = floor_points(sph, lts, np.random.default_rng(7), n=N_FLOOR)
    if cells.shape == (1, 1):  # the fallback: one all-ones word for the whole floor
        have = bits(np.broadcast_to(cells.astype(np.uint32)[0, 0], (len(p),)))
    else:
        have = bits(cell_masks(cells, p, cell))
    n = np.broadcast_to(np.array([0, 1, 0], F), p.shape)
    for sign in (1, -1):
        need, _ = query_needs(p, n, sign, sph, lts)
        lost = need & ~have
        assert not lost.any(), (name, "floor", sign, int(lost.sum()), p[lost.any(axis=(1, 2))][:3])
    rng = np.random.default_rng(11)
    for k in range(4):
        u = rng.normal(size=(N_SPHERE, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        q = (sph[k, :3][None, :] + F(sph[k, 3]) * u.astype(F)).astype(F)
        d = (q - sph[k, :3][None, :]).astype(F)
        nq = (d / np.sqrt(dot(d, d)).astype(F)[:, None]).astype(F)
        have_k = bits(np.uint32(rows[k]))
        for sign in (1, -1):
            need, _ = query_needs(q, nq, sign, sph, lts)
            lost = need & ~have_k[None]
            assert not lost.any(), (name, k, sign, np.argwhere(lost.any(axis=0)))


def test_the_seeds_are_not_vacuous():
    """At least half of the seeds cull with their spans, have floor-class tiles, and get masks
    without the all-ones fallback."""
    culls = classed = masked = 0
    for seed in R.SEEDS:
        case = R.random_ubo(seed)
        ubos = _walk(case)
        p = case.params()
        culls += not is_full(spans(p, ubos), case.width)
        iv = intervals(p, ubos)
        classed += iv is not None and floor_tiles(*iv) > 0
        sph, lts = case.geometry()
        masked += not masks(sph, lts, flags=case.flags)[2]
    n = len(R.SEEDS)
    print(f"of {n} seeds: {culls} with a span that is not full, {classed} with floor-class tiles, {masked} with masks")
    assert 2 * culls >= n and 2 * classed >= n and 2 * masked >= n


def test_every_kind_of_ray_is_traced():
    """Summed over the set, the oracle traces secondary rays, shadow rays and misses."""
    tot = {"secondary_rays": 0, "shadow_rays": 0, "misses": 0}
    for name, case in ALL.items():
        for depth in _depths(name):
            st = _STATS.get((name, depth))
            if st is None:
                st = orc.render(case.scene(), case.params(max_depth=depth))[2]
            for k in tot:
                tot[k] += st[k]
    assert all(v > 0 for v in tot.values()), tot


def test_the_first_of_two_identical_spheres_wins():
    """Strict `<` in scene_intersect: with the second of two identical spheres given the first's
    material too, whichever wins looks the same, and that frame is the case's frame bit for bit."""
    case = R.CASES["duplicate_spheres_first_wins"]
    assert (case.ubo["sphere0"]["center_radius"] == case.ubo["sphere1"]["center_radius"]).all()
    assert case.ubo["sphere0"]["material"] != case.ubo["sphere1"]["material"]
    u = case.ubo.copy()
    u["sphere1"]["material"] = u["sphere0"]["material"]
    a = orc.render(case.scene(), case.params(), want32=True)[1]
    b = orc.render(case.scene(u), case.params(), want32=True)[1]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    u["sphere0"]["material"] = case.ubo["sphere1"]["material"]  # and the second's material would show
    u["sphere1"]["material"] = case.ubo["sphere1"]["material"]
    assert not np.array_equal(a, orc.render(case.scene(u), case.params(), want32=True)[1])
