"""The adversarial meshes of tests/mesh_cases.py on the CPU: each case has the property it is there
for (the 4-wide stack bound that makes the runtime fall back to the binary walk, quantized nodes,
spatial-split duplicates, no BVH at all), the oracle is a usable referee on it (finite, literal and
fast restatements equal bit for bit, enough nearest-triangle hits), the host build is conservative
on it, and the deep-stack ray sets are deep: the kernel's three walks restated in numpy over the
exported nodes hold more entries than the LDS part of the traversal stack, and the triangle a hit
set hits is reached through an entry of the private tail.  tests/test_gpu_mesh_cases.py renders
the same cases and replays the same rays on the GPU.

What the occupancy proofs found (restated walks, `best` = scene_intersect's 1e10):
  binary fallback (LDS 24)   28 entries, nested136 (4-wide bound 68, BVH2 depth 28); the hit of
                             binary_across is reached through entry 26
  4-wide float walk (LDS 24) 47 entries, nested100 (bound 50); 25 on wall46 (bound 27); the hit of
                             wide_across is reached through entry 46
  quantized walk (LDS 16)    47 to 50 entries, nested100; 25 on wall46; hits reached through
                             entries 46 and above (wide_across) and 21 (wall_hit)
All three tails are reachable.  A planar fan spaced along the ray's direction cannot do it: boxes beyond 1e10 are never entered, and the boxes' 1e-6 padding merges everything
below it, which leaves about 53 octaves and a chain of 14 to 18 levels.

The quantized restatement found a kernel bug before any GPU run: with an exact zero in a ray's
direction (culling reciprocal 1e30) and a node origin more than 3.4e8 from the ray's, visit4q's
origin term overflowed to an infinity that put the far plane at -inf and culled children the float
boxes enter (wide_across: 39 of 100 visited references lost).  trt_kernel.hip quant_origin_term
turns the overflow into a NaN, which the slab test ignores; walk4q restates the fixed test."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as orc
from tests import mesh_cases as M
from tests.query_common import expected_hits
from tests.test_bvh_layout import assert_every_triangle_point_is_inside_a_leaf_path
from vkcomputeshader_tinyraytracer_amd import types as T

WALKS = {"binary": M.walk2, "wide": M.walk4, "quant": M.walk4q}


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_the_build_is_what_the_case_is_for(name):
    case = M.CASES[name]
    sc = case.scene
    st = M.diag_build(sc)
    if not case.bvh:
        assert st is None and M.export_bvh2(sc) is None  # "invalid": the batch walk traces it
        assert not np.isfinite(sc.tris["v1"]).all()
        return
    print(name, len(sc.tris), "triangles", len(sc.models), "batches", st)
    assert st["quantized"] == 1 and st["refs"] >= len(sc.tris)
    assert 1 <= st["depth"] <= M.K_BVH_STACK
    assert (st["stack"] > M.K_BVH_STACK) == case.fallback, st
    for k, v in case.expect.items():
        assert st[k] == v, (k, st)
    if case.split:
        assert st["refs"] > len(sc.tris), st
    nodes4, bound = M.export_bvh4(sc)
    assert bound == st["stack"] and len(nodes4) == st["bvh4"]


def test_the_table_is_covered():
    """Batch sizes, triangle counts, flat boxes and degenerate shares the cases are meant to have."""
    many = M.CASES["many_models_b7"].scene
    assert len(many.tris) == 7680 and 1000 < len(many.models) < 1200
    assert (many.models["params0"][:, 1] <= 7).all()
    assert len(M.CASES["soup_loguniform"].scene.tris) == 600 and len(M.CASES["needles"].scene.tris) == 200
    for name, axis in (("flat_on_floor", 1), ("flat_z", 2), ("flat_x_through_camera", 0)):
        sc = M.CASES[name].scene
        assert len(sc.tris) == 128
        for k in ("v0", "v1", "v2"):
            assert np.ptp(sc.tris[k][:, axis]) == 0
    assert (M.CASES["flat_on_floor"].scene.tris["v0"][:, 1] == -4).all()
    deg = M.CASES["degenerate_mix"].scene.tris
    v0, v1, v2 = (deg[k][:, :3].astype(np.float64) for k in ("v0", "v1", "v2"))
    area = np.linalg.norm(np.cross(v1 - v0, v2 - v0), axis=1)
    points = (v0 == v1).all(1) & (v0 == v2).all(1)
    assert points.sum() == 16 and (area < 1e-5).sum() == 32 and (area > 0.1).sum() == 32
    far = M.CASES["far_1e6"].scene.tris["v0"][:, 0]
    assert far.min() > 9e5 and np.spacing(np.float32(1e6)) == 0.0625


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_oracle_modes_agree_and_are_finite(name):
    case = M.CASES[name]
    sc = case.scene
    for depth in M.DEPTHS:
        p = case.params(max_depth=depth)
        a8, a32, ast = orc.render(sc, p, mode=orc.MODE_FAST, want32=True)
        b8, b32, bst = orc.render(sc, p, mode=orc.MODE_LITERAL, want32=True)
        assert np.isfinite(a32).all() and np.isfinite(b32).all(), depth
        assert np.array_equal(a8, b8), depth
        assert np.array_equal(a32.view(np.uint32), b32.view(np.uint32)), depth
        assert ast == bst, depth
        assert ast["primary_rays"] == M.W * M.H
        print(name, depth, "tri_nearest", ast["tri_nearest"])
        assert ast["tri_nearest"] >= case.min_hits.get(depth, 1), (depth, ast)


@pytest.mark.parametrize("name", sorted(n for n, c in M.CASES.items() if c.bvh))
def test_every_triangle_point_is_inside_a_leaf_path(name):
    assert_every_triangle_point_is_inside_a_leaf_path(M.CASES[name].scene)


@pytest.mark.parametrize("name", sorted({d.scene.name: n for n, d in M.DEEP.items()}.values()))
def test_deep_meshes_are_conservative(name):
    assert_every_triangle_point_is_inside_a_leaf_path(M.DEEP[name].scene)


@pytest.mark.parametrize("name", sorted(M.DEEP))
def test_deep_rays_are_deep(name):
    """Every ray of the set's own holds more entries than the LDS part in each walk the set names
    (a condition of the set: never loosened to make a case pass); the walks the runtime takes for
    the mesh are the named ones; the oracle says the rays hit what the set says; and the leaf of a
    hit is reached through an entry of the private tail.  Until that leaf the real walk is the
    restated one.  wall_hit: the oracle's hit is the nearest and the walk goes near to far, so no
    triangle visited before it is hit and `best` is still 1e10.  The across sets: every triangle
    is hit at one t (triangle 0 wins the ties), and the walk restated with `best` at that t from
    the start visits the same nodes with the same stack."""
    ds = M.DEEP[name]
    sc = ds.scene
    st = M.diag_build(sc)
    fallback = st["stack"] > M.K_BVH_STACK
    assert fallback == (ds.beyond == ("binary",)), st
    nodes2, refs = M.export_bvh2(sc)
    nodes4, _ = M.export_bvh4(sc)
    tri_of = refs[:, 9]
    cam = sc.ubo["camPos"][:3]
    own = M.deep_index()
    want = expected_hits(sc, ds.qrays(own))
    dirs = np.unique(ds.rays["dir"][own, :3], axis=0)
    assert len(dirs) >= 5
    if ds.hit_tri is None:
        assert (want["kind"] != T.HIT_TRIANGLE).all()
    else:
        assert (want["kind"] == T.HIT_TRIANGLE).all() and (want["index"] == ds.hit_tri).all()
    for walk in ds.beyond:
        tops, vias = [], []
        for d in dirs:
            top, visits = WALKS[walk](nodes2 if walk == "binary" else nodes4, cam, d)
            tops.append(top)
            if name.endswith("across"):  # ties: every box is entered below the one t of all the hits
                t_hit = want["t"][(ds.rays["dir"][own, :3] == d).all(1)].min()
                assert WALKS[walk](nodes2 if walk == "binary" else nodes4, cam, d, best=t_hit) == (top, visits)
            if walk in ds.via_tail:
                via = [sp for sp, leaf in visits
                       if ds.hit_tri in tri_of[(leaf & M.FMASK):(leaf & M.FMASK) + ((leaf >> M.CSHIFT) & 15) + 1]]
                assert via and None not in via, (walk, d)
                vias.append(min(via))
        print(name, walk, "occupancy", min(tops), "to", max(tops), "hit through entry", min(vias) if vias else None)
        assert min(tops) > M.LDS_OF[walk], (walk, tops)
        assert max(tops) <= M.K_BVH_STACK
        if vias:
            assert min(vias) >= M.LDS_OF[walk], (walk, vias)


def test_the_quantized_walk_visits_what_the_float_walk_visits():
    """Conservativeness of the quantized slab test at the place it was wrong: the across rays (an
    exact zero in the direction, nodes 1e30 wide) visit every leaf reference in the quantized
    restatement that they visit in the float one."""
    ds = M.DEEP["wide_across"]
    nodes4, _ = M.export_bvh4(ds.scene)
    cam = ds.scene.ubo["camPos"][:3]

    def leaves(visits):
        return {k for _, leaf in visits for k in range(leaf & M.FMASK, (leaf & M.FMASK) + ((leaf >> M.CSHIFT) & 15) + 1)}

    for d in np.unique(ds.rays["dir"][M.deep_index(), :3], axis=0)[::6]:
        fl, qu = leaves(M.walk4(nodes4, cam, d)[1]), leaves(M.walk4q(nodes4, cam, d)[1])
        assert len(fl) >= 100 and fl <= qu, (d, len(fl), len(qu))
