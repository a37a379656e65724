"""GPU parity against the CPU oracle on scenes that are not the reference's (tests/random_scenes.py):
drawn and hand-made sphere geometry, materials, lights, cameras and fovs, through every way a frame
is launched that computes a proof from the UBO (sky spans, sphere intervals, shadow occluder masks,
floor class, dark-shadow skip), and through views, samples, meshes, deferred and split frames, and
ray queries.  tests/test_random_scenes.py shows on the CPU that the oracle is a usable referee on
these scenes.  Bars: tests/helpers.py; counters exactly equal.  Run with `pytest -m gpu`."""
from __future__ import annotations

import copy

import numpy as np
import pytest

from oracle import oracle as orc
from tests import helpers, random_scenes as R
from tests.floor_class_common import intervals
from tests.helpers import assert_float_close, assert_rgba8_close
from tests.query_common import expected_hits, oracle_colours, random_rays
from tests.test_gpu_parity import _check
from vkcomputeshader_tinyraytracer_amd import Renderer, scene as S, types as T

pytestmark = pytest.mark.gpu

MAX_FRAC = helpers.MAX_FRAC if R.MAX_FRAC is None else R.MAX_FRAC
ALL = R.all_cases()
SINGLE = [(f"seed{s}", R.seed_depth(s)) for s in R.SEEDS] + [(n, d) for n in R.CASES for d in R.CASE_DEPTHS]
N_WALK = 5  # an odd count: the last frame pair of a launch is half empty
KNOBS = ("TRT_SKY_TABLE", "TRT_SKY_SPANS", "TRT_SKY_SPAN_FRAMES", "TRT_SHADOW_MASK", "TRT_SHADOW_MASK_CELL",
         "TRT_FLOOR_CLASS")
V1 = S.view_ypr(20, -10, 5)
VIEW_SEEDS = (2, 5, 11)
SPP_SEEDS = (3, 8)
# four seeds (the oracle's nearest hit is a triangle for 100 to 1100 rays of each) and the skip's own cases
MESH = ("seed6", "seed9", "seed22", "seed24", "specular_only", "black_sphere")
DEEP_MESH = ("seed6", "seed22", "specular_only", "black_sphere")  # two of the seeds, and the skip's own cases
PINHOLE_SEEDS = (1, 4, 9, 30)
QUERY_SEEDS = (4, 9)
_BASE = R.Case("base", S.make_ubo()).scene()  # binding 4 (the envmap) of every scene here; no meshes
_ORACLE: dict = {}


def _walk(case):
    return S.camera_path(case.ubo, N_WALK, R.WALK_SPEED)


def _runs_with_spans(case) -> bool:
    return intervals(case.params(), _walk(case)) is not None


# the fast family: every seed, and the hand-made cases whose launch runs with spans
WALKS = [(f"seed{s}", R.seed_depth(s)) for s in R.SEEDS] + [(n, 4) for n, c in R.CASES.items() if _runs_with_spans(c)]


def _oracle(case, ubo, p, key):
    """(rgba8, rayOut, counters) of the oracle, computed once per key and never written to."""
    if key not in _ORACLE:
        o8, o32, st = orc.render(case.scene(ubo), p, want32=True)
        o8.setflags(write=False)
        o32.setflags(write=False)
        _ORACLE[key] = (o8, o32, st)
    return _ORACLE[key]


def _exact(st):
    return {k: st[k] for k in T.Stats.EXACT}


def _restore(r):
    r.set_view(None)
    r.set_stream(None)
    r.set_frame_batch(0)
    r.set_frames_in_flight(0)
    r.set_deferred_shadows(0)
    r.set_subtree_split(0)
    if r.scene is not None:
        r.update_ubo(r.scene.ubo)


@pytest.fixture
def r(gpu_renderer):
    """The session's context, handed back as it was found."""
    yield gpu_renderer
    _restore(gpu_renderer)


@pytest.fixture(scope="module")
def no_sky_table(gpu_renderer):
    """A context created under TRT_SKY_TABLE=0 (trace_kernel: no table, spans, masks or class); the
    knobs are read when a context is created."""
    with pytest.MonkeyPatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        mp.setenv("TRT_SKY_TABLE", "0")
        made = Renderer(gpu_renderer.device)
    try:
        yield made
    finally:
        made.close()


def _use(r, ubo):
    if r.scene is not _BASE:
        r.upload_scene(_BASE)
    r.update_ubo(ubo)
    return r


def _check_frame(r, case, p, key, ubo=None):
    """draw_frame against the oracle: both outputs within the bars, counters equal, and the plain
    launch byte-equal to the counting one."""
    ubo = case.ubo if ubo is None else ubo
    _use(r, ubo)
    c8, c32, cst = r.draw_frame(p, count=True, want32=True)
    g8, g32, _ = r.draw_frame(p, want32=True)
    o8, o32, ost = _oracle(case, ubo, p, key)
    assert _exact(cst) == _exact(ost), (cst, ost)
    assert_rgba8_close(c8, o8, max_frac=MAX_FRAC)
    assert_float_close(c32, o32)
    assert g8.tobytes() == c8.tobytes() and g32.tobytes() == c32.tobytes()
    return cst


# ---- a: single frames ---------------------------------------------------------------------------


@pytest.mark.parametrize("name,depth", SINGLE, ids=[f"{n}-d{d}" for n, d in SINGLE])
def test_single_frame(r, name, depth):
    case = ALL[name]
    st = _check_frame(r, case, case.params(max_depth=depth), (name, depth, 0))
    assert st["primary_rays"] == case.width * case.height
    if name == "black_sphere":  # the dark-shadow skip on a sphere
        assert 0 < st["shadow_skipped"] < st["shadow_rays"]


# ---- b: the fast family -------------------------------------------------------------------------


def _frames(r, p, ubos, batch, in_flight):
    import torch

    n = len(ubos)
    out = torch.zeros((n, p.height, p.width, 4), dtype=torch.uint8, device=f"cuda:{r.device}")
    torch.cuda.synchronize(r.device)  # the fill runs on torch's stream, the frames on the context's
    r.set_frame_batch(batch)
    r.set_frames_in_flight(in_flight)
    try:
        r.render_frames(p, out, n, ubos=ubos, frame_stride=p.height * p.width * 4)
        r.synchronize()
    finally:
        r.set_frame_batch(0)
        r.set_frames_in_flight(0)
    return out.cpu().numpy()


@pytest.mark.parametrize("batch,in_flight", [(0, 1), (1, 2)], ids=["pairs", "one-by-one"])
@pytest.mark.parametrize("name,depth", WALKS, ids=[n for n, _ in WALKS])
def test_walk(r, no_sky_table, name, depth, batch, in_flight):
    """A 5-frame walk through render_frames: every frame against the oracle's frame of its UBO,
    byte-equal to draw_frame of it and to the same launch of a TRT_SKY_TABLE=0 context."""
    case = ALL[name]
    p = case.params(max_depth=depth)
    ubos = _walk(case)
    _use(r, case.ubo)
    a = _frames(r, p, ubos, batch, in_flight)
    _use(no_sky_table, case.ubo)
    assert np.array_equal(a, _frames(no_sky_table, p, ubos, batch, in_flight)), "differs from TRT_SKY_TABLE=0"
    for k in range(N_WALK):
        o8 = _oracle(case, ubos[k], p, (name, depth, k))[0]
        assert_rgba8_close(a[k], o8, max_frac=MAX_FRAC)
        r.update_ubo(ubos[k])
        assert np.array_equal(a[k], r.draw_frame(p)[0]), k


# ---- c: views -----------------------------------------------------------------------------------


@pytest.mark.parametrize("seed", VIEW_SEEDS)
def test_view(r, seed):
    """kernel(view) against the oracle fed the host twin's rays, as tests/test_gpu_view.py does."""
    case = R.random_ubo(seed)
    p = case.params(max_depth=R.seed_depth(seed))
    _use(r, case.ubo)
    plain8 = r.draw_frame(p)[0]
    r.set_view(V1)
    c8, c32, cst = r.draw_frame(p, count=True, want32=True)
    g8, g32, _ = r.draw_frame(p, want32=True)
    r.set_view(None)
    rays = S.view_rays(p, V1)
    q = T.Params.from_buffer_copy(p)
    q.rays_in = rays.ctypes.data
    o8, o32, ost = orc.render(case.scene(), q, want32=True)
    assert _exact(cst) == _exact(ost), (cst, ost)
    assert_rgba8_close(c8, o8, max_frac=MAX_FRAC)
    assert_float_close(c32, o32)
    assert g8.tobytes() == c8.tobytes() and g32.tobytes() == c32.tobytes()
    assert not np.array_equal(g8, plain8)


# ---- d: samples ---------------------------------------------------------------------------------


@pytest.mark.parametrize("seed", SPP_SEEDS)
def test_four_samples(r, seed):
    case = R.random_ubo(seed)
    st = _check_frame(r, case, case.params(max_depth=R.seed_depth(seed), spp=4), (case.name, "spp4"))
    assert st["primary_rays"] == 4 * case.width * case.height


# ---- e: meshes ----------------------------------------------------------------------------------


def _mesh_scene(case, depth):
    sc = copy.copy(S.config_c3(case.width, case.height, env_size=R.ENV, level=2))
    sc.ubo = case.ubo
    sc.max_depth = depth
    sc.flags = case.flags
    return sc


@pytest.mark.parametrize("name", MESH)
def test_mesh_scene(r, name):
    """The spheres beside a 320-triangle glass icosphere: the BVH and the reference-order batch
    walk against the oracle, and the plain launches (which skip dark shadow queries) byte-equal to
    the counting ones (which trace them)."""
    case = ALL[name]
    sc = _mesh_scene(case, 4)
    p = case.params(max_depth=4)
    rep, st = _check(r, sc, p, max_frac=MAX_FRAC)
    assert st["tri_nearest"] > 0
    for flags in (p.flags, p.flags | T.FLAG_BATCH_WALK):
        q = case.params(max_depth=4, flags=flags)
        c8, c32, _ = r.draw_frame(q, want32=True, count=True)
        g8, g32, _ = r.draw_frame(q, want32=True)
        assert g8.tobytes() == c8.tobytes() and g32.tobytes() == c32.tobytes()


@pytest.mark.parametrize("name", DEEP_MESH)
def test_mesh_scene_deferred_and_split(r, name):
    """Depth 20 with deferred shadows forced on (bit-equal to the unsplit per-pixel loop, which is
    held to the oracle) and with a subtree-split window of 3 (against the oracle's split mode)."""
    case = ALL[name]
    sc = _mesh_scene(case, 20)
    p = case.params(max_depth=20)
    r.upload_scene(sc)
    o8, o32, ost = orc.render(sc, p, want32=True)

    r.set_deferred_shadows(1)  # off: the per-pixel loop
    r.set_subtree_split(1)
    u8, u32, ust = r.draw_frame(p, want32=True, count=True)
    assert _exact(ust) == _exact(ost), (ust, ost)
    assert_rgba8_close(u8, o8, max_frac=MAX_FRAC)
    assert_float_close(u32, o32)
    g8, g32, _ = r.draw_frame(p, want32=True)  # the plain launch skips dark shadow queries
    assert g8.tobytes() == u8.tobytes() and g32.tobytes() == u32.tobytes()
    r.set_deferred_shadows(2)  # forced on
    d8, d32, _ = r.draw_frame(p, want32=True)
    assert np.array_equal(d8, u8) and np.array_equal(d32, u32)

    r.set_deferred_shadows(1)
    r.set_subtree_split(3)
    s8, s32, sst = r.draw_frame(p, want32=True, count=True)
    w8, w32, wst = orc.render(sc, p, mode=orc.mode_split(3), want32=True)
    assert _exact(sst) == _exact(wst) == _exact(ost), (sst, wst)
    assert_rgba8_close(s8, w8, max_frac=MAX_FRAC)
    assert_float_close(s32, w32)
    g8, g32, _ = r.draw_frame(p, want32=True)
    assert g8.tobytes() == s8.tobytes() and g32.tobytes() == s32.tobytes()


# ---- f: queries ---------------------------------------------------------------------------------


@pytest.mark.parametrize("seed", PINHOLE_SEEDS)
def test_pinhole_query_equals_the_frame(r, seed):
    case = R.random_ubo(seed)
    p = case.params(max_depth=R.seed_depth(seed))
    _use(r, case.ubo)
    want8, want32, wst = r.draw_frame(p, count=True, want32=True)
    rays = S.pinhole_qrays(p, None, case.cam()).reshape(-1)
    g8, g32, _, gst = r.trace_rays(rays, p, count=True, want32=True)
    assert g8.tobytes() == want8.reshape(-1, 4).tobytes()
    assert g32.tobytes() == want32.reshape(-1, 4).tobytes()
    assert _exact(gst) == _exact(wst)


@pytest.fixture(scope="module")
def query_refs():
    """Per query seed: the scene, 1027 free rays, and the oracle's colours, counters and records."""
    out = {}
    for seed in QUERY_SEEDS:
        case = R.random_ubo(seed)
        sc = case.scene()
        p = case.params()
        rays = random_rays(1027, 500 + seed)
        out[seed] = (case, p, rays, oracle_colours(orc._Bound(sc), p, rays), expected_hits(sc, rays))
    return out


@pytest.mark.parametrize("seed", QUERY_SEEDS)
def test_free_rays_match_the_oracle(r, query_refs, seed):
    case, p, rays, (ref8, ref32, tot), _ = query_refs[seed]
    _use(r, case.ubo)
    g8, g32, _, st = r.trace_rays(rays, p, count=True, want32=True)
    assert _exact(st) == {k: tot[k] for k in T.Stats.EXACT}
    assert_rgba8_close(g8, ref8, max_frac=MAX_FRAC)
    assert_float_close(g32, ref32)


@pytest.mark.parametrize("seed", QUERY_SEEDS)
def test_hit_records(r, query_refs, seed):
    case, p, rays, _, want = query_refs[seed]
    _use(r, case.ubo)
    _, _, got, _ = r.trace_rays(rays, p, want8=False, want_hits=True)
    kinds = {k: int((want["kind"] == k).sum()) for k in (T.HIT_NONE, T.HIT_FLOOR, T.HIT_SPHERE)}
    assert all(kinds.values()), kinds
    for k in ("t", "kind", "index", "n"):
        assert got[k].tobytes() == want[k].tobytes(), k
