"""GPU parity against the CPU oracle on the adversarial meshes of tests/mesh_cases.py, through every
copy of the mesh walks: the quantized BVH (GEOM 3, the 5-wave build at depth 4 and the 4-wave build
at depth 6), the unquantized BVH of a context created under TRT_BVH_WAVES4=0 (GEOM 2: the 4-wide
float walk, or the binary fallback when the 4-wide stack bound is above kBvhStack), the
reference-order batch walk (GEOM 1), deferred shadows, the subtree split, sample lanes and the
query kernels; and the deep-stack ray sets replayed through rays_in, whose depth
tests/test_mesh_cases.py proves on the CPU.  Bars: tests/helpers.py; counters exactly equal.  Run
with `pytest -m gpu`.

A GPU result that differs from the oracle here is a bug of the kernel or of the host build: the
oracle restates the shader, and the BVH may only cull."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as orc
from tests import helpers, mesh_cases as M
from tests.helpers import assert_float_close, assert_rgba8_close
from tests.query_common import expected_hits, f32, oracle_colours, random_rays
from tests.test_gpu_parity import _check
from tests.test_gpu_query import _check_mesh_path
from vkcomputeshader_tinyraytracer_amd import Renderer, types as T

pytestmark = pytest.mark.gpu

MAX_FRAC = helpers.MAX_FRAC if M.MAX_FRAC is None else M.MAX_FRAC
FRAMES = [(n, d) for n in M.CASES for d in M.DEPTHS]


def _exact(st, keys=T.Stats.EXACT):
    return {k: st[k] for k in keys}


def _walk_counters(st):
    """Every counter of a frame (not its time): equal when the same kernel walks the same nodes."""
    return {k: v for k, v in st.items() if k != "kernel_ms"}


def _restore(r):
    r.set_view(None)
    r.set_stream(None)
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
def g2(gpu_renderer):
    """A context created under TRT_BVH_WAVES4=0: mesh scenes take the GEOM 2 kernels (the knob is
    read when a context is created)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("TRT_BVH_WAVES4", "0")
        made = Renderer(gpu_renderer.device)
    try:
        yield made
    finally:
        made.close()


def _plain_equals_counting(r, p):
    for flags in (p.flags, p.flags | T.FLAG_BATCH_WALK):
        q = T.Params.from_buffer_copy(p)
        q.flags = flags
        c8, c32, _ = r.draw_frame(q, want32=True, count=True)
        g8, g32, _ = r.draw_frame(q, want32=True)
        assert g8.tobytes() == c8.tobytes() and g32.tobytes() == c32.tobytes(), flags


# ---- the fallback walk, first: it has not run on a GPU before this file ---------------------------


def test_fallback_walk_first(r):
    """fan_stepped_b2 at depth 4: the 4-wide stack bound is 66, so the frame runs GEOM 2 without
    4-wide nodes, the binary walk (nearest hit and shadow), against the oracle."""
    case = M.CASES["fan_stepped_b2"]
    assert case.fallback
    rep, st = _check(r, case.scene, case.params(max_depth=4), max_frac=MAX_FRAC)
    assert st["tri_nearest"] > 0


# ---- every case at depth 4 and 6 ------------------------------------------------------------------


@pytest.mark.parametrize("name,depth", FRAMES, ids=[f"{n}-d{d}" for n, d in FRAMES])
def test_frame(r, name, depth):
    """_check: the BVH frame against the oracle (computed here, once per case and depth), the
    batch walk byte-equal to it with the reference's batch and triangle work; then the plain
    launches byte-equal to the counting ones."""
    case = M.CASES[name]
    p = case.params(max_depth=depth)
    rep, st = _check(r, case.scene, p, max_frac=MAX_FRAC)
    assert st["primary_rays"] == M.W * M.H
    assert st["tri_nearest"] >= case.min_hits.get(depth, 1)
    _plain_equals_counting(r, p)


@pytest.mark.parametrize("name", list(M.CASES))
def test_geom2_context(r, g2, name):
    """The frame of a TRT_BVH_WAVES4=0 context is the default context's, byte for byte, with the
    EXACT counters equal; a fallback case (and the case without a BVH) runs the same kernel from
    both contexts, so every counter is equal."""
    case = M.CASES[name]
    p = case.params(max_depth=6)
    r.upload_scene(case.scene)
    g2.upload_scene(case.scene)
    a8, a32, ast = r.draw_frame(p, want32=True, count=True)
    b8, b32, bst = g2.draw_frame(p, want32=True, count=True)
    assert a8.tobytes() == b8.tobytes() and a32.tobytes() == b32.tobytes()
    assert _exact(ast) == _exact(bst)
    if case.fallback or not case.bvh:
        assert _walk_counters(ast) == _walk_counters(bst)
    _plain_equals_counting(g2, p)


def test_inverted_batch_box(r):
    """A Model record with bboxMin > bboxMax on an axis: the reference's slab test orders the two
    planes per axis, so it is the same box, and the batch walk's hierarchy (unions of batch boxes)
    must not take it for an empty one.  flat_z's second batch (the rows y >= 1) with its y planes
    swapped: the union of the two batches took y in [-4, 1] and the walk lost the upper half of the
    mesh.  fan_overflow's last batch is the builder's own case of it: every vertex NaN on y and z,
    so its box keeps the FLT_MAX / -FLT_MAX sentinels there, and the reference enters it."""
    import copy

    sc = copy.copy(M.CASES["flat_z"].scene)
    sc.models = sc.models.copy()
    assert len(sc.models) == 2
    lo, hi = float(sc.models[1]["bboxMin"][1]), float(sc.models[1]["bboxMax"][1])
    assert lo < hi
    sc.models[1]["bboxMin"][1], sc.models[1]["bboxMax"][1] = hi, lo
    p = sc.params(max_depth=4)
    rep, st = _check(r, sc, p, max_frac=MAX_FRAC)
    r.upload_scene(M.CASES["flat_z"].scene)
    assert r.draw_frame(p, want32=True, count=True)[2]["tri_nearest"] == st["tri_nearest"]


# ---- the deep-stack rays ---------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(M.DEEP))
def test_deep_rays_replayed(r, g2, name):
    """A deep set through rays_in on the walk the default context takes for its mesh (quantized,
    or the binary fallback) and on the GEOM 2 context's (4-wide float, or the same fallback),
    against the oracle fed the same rays: counters exact, both outputs within the bars, the plain
    launch and the batch walk byte-equal.  The rays of a hit set hit the set's triangle (the hit
    records of the query kernels' copies of the walks say which), reached through the private
    tail: a wrong pop is a wrong hit, and triangle 0 of the nested meshes has its own material."""
    ds = M.DEEP[name]
    sc = ds.scene
    p = ds.params(max_depth=4)
    q = T.Params.from_buffer_copy(p)
    q.rays_in = ds.rays.ctypes.data
    o8, o32, ost = orc.render(sc, q, want32=True)
    own = M.deep_index()
    qrays = ds.qrays()
    want = expected_hits(sc, qrays)
    if ds.hit_tri is None:
        assert (want["kind"][own] != T.HIT_TRIANGLE).all()
    else:
        assert (want["kind"][own] == T.HIT_TRIANGLE).all() and (want["index"][own] == ds.hit_tri).all()
        assert ost["tri_nearest"] >= len(own)
    frames = []
    for ctx in (r, g2):
        ctx.upload_scene(sc)
        c8, c32, cst = ctx.draw_frame(p, rays_in=ds.rays, want32=True, count=True)
        assert _exact(cst) == _exact(ost), (cst, ost)
        assert_rgba8_close(c8, o8, max_frac=MAX_FRAC)
        assert_float_close(c32, o32)
        g8, g32, _ = ctx.draw_frame(p, rays_in=ds.rays, want32=True)
        assert g8.tobytes() == c8.tobytes() and g32.tobytes() == c32.tobytes()
        pw = T.Params.from_buffer_copy(p)
        pw.flags |= T.FLAG_BATCH_WALK
        w8, w32, wst = ctx.draw_frame(pw, rays_in=ds.rays, want32=True, count=True)
        assert _exact(wst, T.Stats.EXACT_WALK) == _exact(ost, T.Stats.EXACT_WALK), (wst, ost)
        assert w8.tobytes() == c8.tobytes() and w32.tobytes() == c32.tobytes()
        # the same rays as a query (which normalizes them once more): records in the shader's own order
        _, _, hits, _ = ctx.trace_rays(qrays, p, want8=False, want_hits=True)
        for k in ("t", "kind", "index", "n"):
            assert hits[k].tobytes() == want[k].tobytes(), k
        _, _, whits, _ = ctx.trace_rays(qrays, pw, want8=False, want_hits=True)
        assert whits.tobytes() == hits.tobytes()
        frames.append((c8, c32, cst))
    assert frames[0][0].tobytes() == frames[1][0].tobytes() and frames[0][1].tobytes() == frames[1][1].tobytes()
    if "binary" in ds.beyond:
        assert _walk_counters(frames[0][2]) == _walk_counters(frames[1][2])


# ---- depth 20: deferred shadows and the subtree split -------------------------------------------


@pytest.mark.parametrize("name", M.DEEP_FRAMES)
def test_deferred_and_split(r, name):
    """Depth 20 with deferred shadows forced on (bit-equal to the unsplit per-pixel loop, which is
    held to the oracle) and with a subtree-split window of 3 (against the oracle's split mode), as
    tests/test_gpu_random_scenes.py::test_mesh_scene_deferred_and_split does it."""
    case = M.CASES[name]
    sc = case.scene
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


# ---- four samples: one lane per sample, the wave-coherent shadow walk ---------------------------


@pytest.mark.parametrize("name", M.SPP_CASES)
def test_four_samples(r, name):
    case = M.CASES[name]
    p = case.params(max_depth=4, spp=4)
    rep, st = _check(r, case.scene, p, max_frac=MAX_FRAC)
    assert st["primary_rays"] == 4 * M.W * M.H and st["tri_nearest"] > 0
    _plain_equals_counting(r, p)


# ---- ray queries with hit records ----------------------------------------------------------------


def _query_rays(sc, seed):
    """1027 free rays; every second one aims at a point drawn inside a triangle drawn from the mesh
    (of those within 100 units that have an area) and starts within 4 units of that point."""
    rays = random_rays(1027, seed)
    rng = np.random.default_rng(seed + 1)
    aim = np.arange(0, len(rays), 2)
    v = np.stack([sc.tris[k][:, :3] for k in ("v0", "v1", "v2")], 1).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        area = np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
    big = np.flatnonzero((area > 1e-3) & (np.abs(v).max(axis=(1, 2)) < 100.0))  # not degenerate, not far away
    pick = v[rng.choice(big, len(aim))]
    w = rng.dirichlet((1.0, 1.0, 1.0), len(aim))
    target = np.einsum("nk,nkc->nc", w, pick)
    org = target + rng.uniform(-4, 4, size=target.shape)
    rays["org"][aim] = org.astype(f32)
    rays["dir"][aim] = (target - rays["org"][aim].astype(np.float64)).astype(f32)
    return rays


@pytest.fixture(scope="module")
def query_refs():
    """Per query case: the rays with the oracle's colours, counters and expected records."""
    out = {}
    for i, name in enumerate(M.QUERY_CASES):
        sc = M.CASES[name].scene
        rays = _query_rays(sc, 7000 + i)
        ref8, ref32, tot = oracle_colours(orc._Bound(sc), sc.params(), rays)
        want = expected_hits(sc, rays)
        assert int((want["kind"] == T.HIT_TRIANGLE).sum()) > 100
        out[name] = (rays, ref8, ref32, tot, want)
    return out


@pytest.mark.parametrize("name", M.QUERY_CASES)
def test_queries_with_hit_records(r, g2, query_refs, name):
    """The query kernels of every mesh path against the same references: the default context's
    walk, the reference-order batch walk and the GEOM 2 context, bit for bit with each other."""
    sc = M.CASES[name].scene
    p = sc.params()
    r.upload_scene(sc)
    a = _check_mesh_path(r, sc, p, query_refs[name], T.Stats.EXACT)
    b = _check_mesh_path(r, sc, sc.params(flags=sc.flags | T.FLAG_BATCH_WALK), query_refs[name], T.Stats.EXACT_WALK)
    g2.upload_scene(sc)
    c = _check_mesh_path(g2, sc, p, query_refs[name], T.Stats.EXACT)
    for other in (b, c):
        for x, y in zip(a, other):
            assert x.tobytes() == y.tobytes()
