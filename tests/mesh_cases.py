"""Adversarial meshes, shared by tests/test_mesh_cases.py (CPU) and tests/test_gpu_mesh_cases.py: the
mechanisms of the BVH build that ordinary meshes never reach — the binary
fallback walk behind a 4-wide stack bound above kBvhStack, the private tail of the traversal stack,
quantized nodes at large coordinate-to-extent ratios, over a wide range of triangle sizes and with
zero-thickness boxes, spatial-split duplicates of very different sizes in one leaf, degenerate
triangles, a mesh in the floor's plane, a mesh plane through the camera, and odd batch sizes.

Every case is the reference's spheres, floor and lights under FLAGS at 72 x 52 with a 256 x 128
envmap; its triangles go through S.SceneBuilder(batch_size).add_mesh, so batches and their boxes
are the product builder's.  All draws are seeded.  No GPU is needed to import this module.

fan_overflow is the fan of base 2 with k up to 129, whose largest vertices round to inf in float32
(the builder's transform then makes their other coordinates NaN: 0 * inf): no BVH is built for it
(trt_diag_bvh_export returns "invalid"), so the batch walk traces it.  Its oracle frame is finite
(NaN terms fail the reference's comparisons, so those triangles are never hit), so it is a case:
the upload succeeds and the frame equals the oracle's.  Its last batch keeps the builder's
FLT_MAX / -FLT_MAX sentinels as its box on y and z, which the reference's slab test enters; the
batch hierarchy took that box for an empty one until this case.

The deep-stack ray sets (DEEP) are replayed through rays_in from the case's camera; the numpy walks
below restate the kernel's three walks over the exported nodes and report the largest number of
stack entries a ray holds, which tests/test_mesh_cases.py asserts is beyond the LDS part."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from vkcomputeshader_tinyraytracer_amd import lib, scene as S, types as T

W, H = 72, 52  # partial 8x8 and 16x16 tiles on both axes
ENV = (256, 128)
FLAGS = T.FLAG_SPHERES | T.FLAG_FLOOR | T.FLAG_ENVMAP | T.FLAG_ROW_QUIRK
DEPTHS = (4, 6)  # 4: the 5-wave shallow build; 6: the 4-wave build

# The parity log of the GPU file (TRT_PARITY_LOG, tests/helpers.py) over these scenes.  Every
# comparison of that log is within 1 LSB and within FLOAT_TOL; the cap on the share of pixels that
# differ by that 1 LSB is helpers.MAX_FRAC unless the log shows that these scenes need their own,
# which is then twice the log's worst fraction and never above 0.02 (the rule helpers.py states).
PARITY_LOG = "profiles/mesh_cases_parity.jsonl"
MAX_FRAC = None  # None: helpers.MAX_FRAC holds

K_BVH_STACK = 64  # trt_device.h kBvhStack
LDS_G3, LDS_G2 = 16, 24  # trt_kernel.hip TRT_G3_LDS, TRT_BVH_LDS_N: stack entries held in LDS


@dataclass
class MeshCase:
    """One scene with what the CPU test asserts of its build and its oracle frame."""

    name: str
    scene: S.Scene
    fallback: bool = False      # 4-wide stack bound > kBvhStack: the runtime walks the BVH2
    split: bool = False         # spatial splits: leaf references > triangles
    min_hits: dict = field(default_factory=dict)  # depth -> least tri_nearest of the oracle frame
    bvh: bool = True            # False: no BVH is built, the batch walk traces the meshes
    expect: dict = field(default_factory=dict)    # exact values of trt_diag_bvh_build

    def params(self, **kw) -> T.Params:
        return self.scene.params(**kw)

    def cam(self) -> tuple:
        return tuple(float(v) for v in self.scene.ubo["camPos"][:3])


def _scene(name, builder, cam=(0.0, 0.0, 0.0)) -> S.Scene:
    tris, models = builder.arrays()
    builder.close()
    return S.Scene(name, S.make_ubo(cam=cam), tris, models, S.cached_envmap(*ENV), W, H, 4, flags=FLAGS)


def _soup_mesh(tri_vertices):
    """(n, 3, 3) vertices -> positions and indices of n separate triangles."""
    v = np.asarray(tri_vertices, np.float64).reshape(-1, 3)
    return v.astype(np.float32), np.arange(len(v), dtype=np.uint32).reshape(-1, 3)


def fan_vertices(base: float, n: int, stepped: bool, k0: int = 0) -> np.ndarray:
    """Triangle k: v0 = (b^k, -3, z), v1 = (1.9 b^k, -3, z), v2 = (b^k, 3, z); z = -10, or
    -6 - 0.02 k when stepped.  Computed in double, rounded once to float32 by the builder."""
    k = np.arange(k0, k0 + n, dtype=np.float64)
    x = np.power(np.float64(base), k)
    z = -6.0 - 0.02 * k if stepped else np.full(n, -10.0)
    v = np.zeros((n, 3, 3))
    v[:, 0] = np.stack([x, np.full(n, -3.0), z], 1)
    v[:, 1] = np.stack([1.9 * x, np.full(n, -3.0), z], 1)
    v[:, 2] = np.stack([x, np.full(n, 3.0), z], 1)
    return v


def _fan(name, base, n, stepped, cam=(0.0, 0.0, 0.0), mat=None, batch=64):
    with np.errstate(over="ignore"):
        pos, idx = _soup_mesh(fan_vertices(base, n, stepped))
    b = S.SceneBuilder(batch)
    b.add_mesh(pos, idx, S.GLASS_MESH_MAT if mat is None else mat, normal_interp=0)
    return _scene(name, b, cam)


def _strip(name, base, n):
    """_strip_scene of tests/test_bvh_layout.py through the builder: triangles 1 wide at x = b^k."""
    x = np.power(np.float64(base), np.arange(n, dtype=np.float64))
    v = np.zeros((n, 3, 3))
    v[:, 0] = np.stack([x, np.zeros(n), np.full(n, -10.0)], 1)
    v[:, 1] = np.stack([x + 1.0, np.zeros(n), np.full(n, -10.0)], 1)
    v[:, 2] = np.stack([x, np.ones(n), np.full(n, -10.0)], 1)
    b = S.SceneBuilder()
    b.add_mesh(*_soup_mesh(v), S.BUNNY_MAT, normal_interp=0)
    return _scene(name, b)


def _far(name, off):
    pos, idx = S.icosphere(2)
    b = S.SceneBuilder()
    b.add_mesh(pos, idx, S.GLASS_MESH_MAT, scale=(1.5, 1.5, 1.5), translation=(off + 2.5, -2.0, -10.0), normal_interp=1)
    return _scene(name, b, cam=(off, 0.0, 0.0))


def _soup(name, n=600, seed=21):
    rng = np.random.default_rng(seed)
    c = rng.uniform((-8, -4, -28), (8, 6, -4), size=(n, 3))
    size = np.power(10.0, rng.uniform(-3, 1, size=n))
    v = c[:, None, :] + rng.normal(size=(n, 3, 3)) * size[:, None, None]
    b = S.SceneBuilder()
    b.add_mesh(*_soup_mesh(v), S.GLASS_MESH_MAT, normal_interp=0)
    return _scene(name, b)


def _needles(name, n=200, seed=22):
    rng = np.random.default_rng(seed)
    a = rng.uniform((-8, -4, -28), (8, 6, -4), size=(n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    e = rng.normal(size=(n, 3))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    v = np.stack([a, a + 12.0 * d, a + 0.05 * e], 1)
    b = S.SceneBuilder()
    b.add_mesh(*_soup_mesh(v), S.DRAGON_MAT, normal_interp=0)
    return _scene(name, b)


def _grid(origin, du, dv, n=8):
    """n x n quads (2 n^2 triangles) spanning origin + [0, n] du + [0, n] dv, shared vertices."""
    o, du, dv = (np.asarray(a, np.float64) for a in (origin, du, dv))
    pos = np.array([o + i * du + j * dv for j in range(n + 1) for i in range(n + 1)], np.float32)
    idx = []
    for j in range(n):
        for i in range(n):
            a, b_, c, d = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i + 1, (j + 1) * (n + 1) + i
            idx += [(a, b_, c), (a, c, d)]
    return pos, np.asarray(idx, np.uint32)


def _flat(name, origin, du, dv, mat):
    b = S.SceneBuilder()
    b.add_mesh(*_grid(origin, du, dv), mat, normal_interp=0)
    return _scene(name, b)


def _degenerate(name, n=64, seed=23):
    rng = np.random.default_rng(seed)
    v = np.zeros((n, 3, 3))
    for k in range(n):
        a = np.array([rng.uniform(-7, 7), rng.uniform(-3, 5), -12.0])
        if k % 4 == 0:  # a point
            v[k] = a
        elif k % 4 == 1:  # collinear
            d = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), 0.0])
            v[k] = (a, a + d, a + 2.0 * d)
        else:
            v[k] = (a, a + (rng.uniform(0.5, 2.5), rng.uniform(-0.5, 0.5), 0.0), a + (rng.uniform(-0.5, 0.5), rng.uniform(0.5, 2.5), 0.0))
    b = S.SceneBuilder()
    b.add_mesh(*_soup_mesh(v), S.WHISKY_MAT, normal_interp=0)
    return _scene(name, b)


def _many_models(name):
    pos, idx = S.icosphere(2)
    mats = (S.GLASS_MESH_MAT, S.BUNNY_MAT, S.VENUS_MAT)
    b = S.SceneBuilder(7)
    for k in range(24):
        gx, gz = k % 6, k // 6
        b.add_mesh(pos, idx, mats[k % 3], scale=(0.4, 0.4, 0.4),
                   translation=(-5.0 + 2.0 * gx, -3.0 + 0.75 * (k % 4), -7.0 - 3.0 * gz), normal_interp=k % 2)
    return _scene(name, b)


def overflowing_fan() -> S.Scene:
    """The fan of base 2 with k up to 129: 2^128 and beyond round to inf in float32."""
    return _fan("fan_overflow", 2.0, 130, True)


def _cases() -> dict:
    c = {}

    def add(name, scene, **kw):
        c[name] = MeshCase(name, scene, **kw)

    add("fan_planar_b2", _fan("fan_planar_b2", 2.0, 120, False), fallback=True,
        expect={"depth": 29, "stack": 73})
    add("fan_stepped_b2", _fan("fan_stepped_b2", 2.0, 120, True), fallback=True, expect={"stack": 66}, min_hits={6: 375})
    add("fan_b13_planar", _fan("fan_b13_planar", 1.3, 100, False), expect={"stack": 35})
    add("fan_b13_stepped", _fan("fan_b13_stepped", 1.3, 100, True), expect={"stack": 34}, min_hits={6: 1226})
    add("strip_b12", _strip("strip_b12", 1.2, 400), fallback=True, expect={"stack": 76})
    add("far_1e4", _far("far_1e4", 1e4), min_hits={4: 282})
    add("far_1e6", _far("far_1e6", 1e6), min_hits={4: 417})
    add("soup_loguniform", _soup("soup_loguniform"), split=True, min_hits={6: 7387})
    add("needles", _needles("needles"), split=True)
    add("flat_on_floor", _flat("flat_on_floor", (-8, -4, -28), (2, 0, 0), (0, 0, 2.75), S.VENUS_MAT), min_hits={6: 9})
    add("flat_z", _flat("flat_z", (-8, -4, -12), (2, 0, 0), (0, 1.25, 0), S.GLASS_MESH_MAT), min_hits={6: 543})
    add("flat_x_through_camera", _flat("flat_x_through_camera", (0, -4, -20), (0, 1, 0), (0, 0, 2), S.BUNNY_MAT),
        min_hits={6: 65})
    add("degenerate_mix", _degenerate("degenerate_mix"), min_hits={6: 136})
    add("many_models_b7", _many_models("many_models_b7"), min_hits={6: 459})
    add("fan_overflow", overflowing_fan(), bvh=False, min_hits={6: 375})
    return c


CASES = _cases()
FALLBACK = tuple(n for n, c in CASES.items() if c.fallback)
DEEP_FRAMES = ("fan_stepped_b2", "soup_loguniform", "flat_z", "many_models_b7")  # depth 20: deferred and split
SPP_CASES = ("soup_loguniform", "fan_b13_stepped")
QUERY_CASES = ("fan_stepped_b2", "soup_loguniform", "degenerate_mix")


# ---- the exported hierarchies -------------------------------------------------------------------

LEAF, CSHIFT, FMASK, NONE = 0x80000000, 27, (1 << 27) - 1, 0xFFFFFFFF


def _arrays(sc):
    return np.ascontiguousarray(sc.tris, T.TRIANGLE), np.ascontiguousarray(sc.models, T.MODEL)


def diag_build(sc):
    """trt_diag_bvh_build: counts of the host build, or None when no BVH is built."""
    L = lib()
    f = L.trt_diag_bvh_build
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
    tris, models = _arrays(sc)
    out = (ctypes.c_uint64 * 6)()
    if f(tris.ctypes.data, len(tris), models.ctypes.data, len(models), out) != 0:
        return None
    return dict(zip(("bvh2", "bvh4", "quantized", "depth", "stack", "refs"), [int(v) for v in out]))


def export_bvh2(sc):
    """trt_diag_bvh_export: (nodes (n, 16) uint32, leaf references (m, 12) uint32), or None."""
    L = lib()
    f = L.trt_diag_bvh_export
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                  ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
    tris, models = _arrays(sc)
    cnt = (ctypes.c_uint64 * 2)()
    if f(tris.ctypes.data, len(tris), models.ctypes.data, len(models), None, 0, None, 0, cnt) != 0:
        return None
    nodes = np.zeros((cnt[0], 16), np.uint32)
    refs = np.zeros((cnt[1], 12), np.uint32)
    assert f(tris.ctypes.data, len(tris), models.ctypes.data, len(models), nodes.ctypes.data, cnt[0],
             refs.ctypes.data, cnt[1], cnt) == 0
    return nodes, refs


def export_bvh4(sc):
    """trt_diag_bvh4_export: (nodes (n, 32) uint32: lox loy loz hix hiy hiz child pad, 4 each; the
    worst-case stack collapse_bvh4 reports)."""
    L = lib()
    f = L.trt_diag_bvh4_export
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                  ctypes.POINTER(ctypes.c_uint64)]
    tris, models = _arrays(sc)
    cnt = (ctypes.c_uint64 * 2)()
    assert f(tris.ctypes.data, len(tris), models.ctypes.data, len(models), None, 0, cnt) == 0
    nodes = np.zeros((cnt[0], 32), np.uint32)
    assert f(tris.ctypes.data, len(tris), models.ctypes.data, len(models), nodes.ctypes.data, cnt[0], cnt) == 0
    return nodes, int(cnt[1])


# ---- the walks, restated ------------------------------------------------------------------------

f32 = np.float32


def cull_inv(d):
    """trt_kernel.hip cull_inv: 1 / d with components below 1e-30 in magnitude made +-1e-30 first."""
    d = np.asarray(d, f32)
    d = np.where(np.abs(d) < f32(1e-30), np.copysign(f32(1e-30), d), d).astype(f32)
    return (f32(1) / d).astype(f32)


def _box(o, inv, lo, hi, best):
    """bvh_box: the slab test with NaN-ignoring min / max; (entered, tnear)."""
    with np.errstate(invalid="ignore", over="ignore"):
        t0 = (lo - o) * inv
        t1 = (hi - o) * inv
        tn = np.fmax(np.fmax(np.fmin(t0[0], t1[0]), np.fmin(t0[1], t1[1])), np.fmin(t0[2], t1[2]))
        tf = np.fmin(np.fmin(np.fmax(t0[0], t1[0]), np.fmax(t0[1], t1[1])), np.fmax(t0[2], t1[2]))
        return bool(tn <= tf and tf > f32(1e-4) and tn <= best), tn


BEST0 = f32(1e10)  # scene_intersect's h.t when neither the floor nor a sphere is hit


def walk2(nodes, o, d, best=BEST0):
    """trace_bvh for a ray that hits no triangle (`best` stays what scene_intersect starts with):
    where both children are entered the nearer becomes the node and the other is pushed.  Returns
    (largest stack occupancy, [(stack index of the latest pop or None, leaf ref)] of the leaves
    visited: a leaf is reached through the entry its latest pop read)."""
    boxes = nodes[:, :12].view(f32).reshape(-1, 4, 3)
    child = nodes[:, 12:14]
    o, inv = np.asarray(o, f32), cull_inv(d)
    stack, node, top, pops, last = [], 0, 0, [], None
    while True:
        if not node & LEAF:
            ha, ta = _box(o, inv, boxes[node, 0], boxes[node, 1], best)
            hb, tb = _box(o, inv, boxes[node, 2], boxes[node, 3], best)
            if ha and hb:
                a_first = ta <= tb
                stack.append(int(child[node, 1 if a_first else 0]))
                top = max(top, len(stack))
                node = int(child[node, 0 if a_first else 1])
                continue
            if ha or hb:
                node = int(child[node, 0 if ha else 1])
                continue
        else:
            pops.append((last, node))
        if not stack:
            return top, pops
        node = stack.pop()
        last = len(stack)


def _sorted_push(t, r, stack):
    """visit4 / visit4q after the box tests: the kernel's network of five compare-exchanges on
    (t, ref) with misses at +inf, the nearest returned, the others pushed farthest first."""
    nh = sum(1 for x in t if x != np.inf)
    if nh == 0:
        return None
    for a, b in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):
        if t[b] < t[a]:
            t[a], t[b], r[a], r[b] = t[b], t[a], r[b], r[a]
    for k in range(nh - 1, 0, -1):
        stack.append(r[k])
    return r[0]


def _walk4(visit, o, d):
    stack, node, top, pops, last = [], 0, 0, [], None
    while True:
        if not node & LEAF:
            nxt = visit(node, stack)
            if nxt is not None:
                top = max(top, len(stack))
                node = nxt
                continue
        else:
            pops.append((last, node))
        if not stack:
            return top, pops
        node = stack.pop()
        last = len(stack)


def walk4(nodes4, o, d, best=BEST0):
    """trace_bvh4 over the float 4-wide nodes (GEOM 2) for a ray that hits no triangle; returns
    what walk2 returns."""
    fl = nodes4[:, :24].view(f32).reshape(-1, 6, 4)  # lox loy loz hix hiy hiz
    child = nodes4[:, 24:28]
    o, inv = np.asarray(o, f32), cull_inv(d)

    def visit(node, stack):
        t, r = [], [int(c) for c in child[node]]
        for i in range(4):
            ok, tn = _box(o, inv, fl[node, 0:3, i], fl[node, 3:6, i], best)
            t.append(tn if ok else f32(np.inf))
        return _sorted_push(t, r, stack)

    return _walk4(visit, o, d)


def quantize4(nodes4):
    """quantize_bvh4 restated: per node (p (3,) float32, step exponents (3,), qlo (3, 4), qhi (3, 4))."""
    fl = nodes4[:, :24].view(f32).reshape(-1, 6, 4).astype(np.float64)
    child = nodes4[:, 24:28]
    n = len(nodes4)
    p = np.zeros((n, 3), f32)
    ex = np.zeros((n, 3), np.int64)
    qlo = np.full((n, 3, 4), 255, np.int64)
    qhi = np.zeros((n, 3, 4), np.int64)
    for i in range(n):
        used = child[i] != NONE
        for a in range(3):
            lo, hi = fl[i, a][used], fl[i, 3 + a][used]
            L, Hh = lo.min(), hi.max()
            ext = max(Hh - L, 1e-30)
            e = int(np.ceil(np.log2(ext / 250.0)))
            while np.ldexp(250.0, e) < ext:
                e += 1
            sd = np.ldexp(1.0, e)
            pd = L - sd
            pf = f32(pd)
            if np.float64(pf) > pd:
                pf = np.nextafter(pf, f32(-np.inf))
            p[i, a], ex[i, a] = pf, e
            ql = np.clip(np.floor((lo - np.float64(pf)) / sd) - 1.0, 0, 255)
            qh = np.clip(np.ceil((hi - np.float64(pf)) / sd) + 1.0, 0, 255)
            assert (np.float64(pf) + ql * sd <= lo).all() and (np.float64(pf) + qh * sd >= hi).all()
            qlo[i, a][used], qhi[i, a][used] = ql, qh
    return p, ex, qlo, qhi


def walk4q(nodes4, o, d, best=BEST0):
    """trace_bvh4 over the quantized nodes (GEOM 3, visit4q) for a ray that hits no triangle: a
    plane's distance is fma(q, s * inv, (p - o) * inv), the fused product computed in double and
    rounded to float32.  Returns what walk2 returns."""
    p, ex, qlo, qhi = quantize4(nodes4)
    child = nodes4[:, 24:28]
    o, inv = np.asarray(o, f32), cull_inv(d)

    def visit(node, stack):
        with np.errstate(over="ignore", invalid="ignore"):
            a = ((p[node] - o) * inv).astype(f32)
            a = np.where(np.isinf(a), f32(np.nan), a)  # quant_origin_term
            b = (np.ldexp(f32(1), ex[node]).astype(f32) * inv).astype(f32)
            t, r = [], [int(c) for c in child[node]]
            for i in range(4):
                near = np.where(inv >= 0, qlo[node, :, i], qhi[node, :, i]).astype(np.float64)
                far = np.where(inv >= 0, qhi[node, :, i], qlo[node, :, i]).astype(np.float64)
                tn3 = (near * b.astype(np.float64) + a.astype(np.float64)).astype(f32)
                tf3 = (far * b.astype(np.float64) + a.astype(np.float64)).astype(f32)
                tn = np.fmax(np.fmax(tn3[0], tn3[1]), tn3[2])
                tf = np.fmin(np.fmin(tf3[0], tf3[1]), tf3[2])
                ok = bool(tn <= tf and tf > f32(1e-4) and tn <= best)
                t.append(tn if ok else f32(np.inf))
        return _sorted_push(t, r, stack)

    return _walk4(visit, o, d)


# ---- deep-stack ray sets ------------------------------------------------------------------------
#
# A traversal stack grows by one entry at every level of a root-to-leaf path at which the ray also
# enters a sibling, so it needs a skewed tree whose siblings all lie on one ray.  Binned SAH peels
# the few largest triangles off a geometrically spaced set at every level (tests/test_bvh_layout.py
# test_bvh_depth_is_bounded), which gives the skew; two families put the siblings on a ray:
#
#   nested  planar triangles (0, -0.1 s, -10), (10, -0.1 s, -10), (0, 2 s, -10) with s = 2^k: the
#           boxes nest around the line y = 0 of the plane, and a ray along that line, inside the
#           plane, enters every one of them at the same distance and hits none (Moller-Trumbore's
#           determinant is exactly 0).  The entry distances tie, which the float walks' restatements
#           reproduce exactly; s spans 2^-16 (the boxes' absolute padding is 1e-6) to 2^119.
#   wall    triangles in the planes x = 2^k, k = -13 .. 32, all crossing the line (y, z) = (0, -10)
#           with their boxes: a ray along +x from x = 0 enters them at distances 2^k, far more than
#           a quantization step apart (nothing beyond 1e10 is entered: scene_intersect's first
#           `best`).  Triangles below WALL_FLIP cover y + (z + 10) <= 0, the others >= 2: a ray at
#           0.5 + 0.5 passes through every box and no triangle, a ray at 1.5 + 1.5 misses the small
#           triangles and hits triangle WALL_FLIP, whose stack entry lies in the private tail.
#
# A ray set is a 72 x 52 frame replayed through rays_in from one camera (every ray starts at
# camPos): every eighth ray is the set's own, tilted by multiples of 1e-11 (it stays inside a 1-unit
# window over 1e10 units), the others are drawn towards the spheres so that the lanes of a wave
# diverge.

WALL_BASE, WALL_K0, WALL_N, WALL_FLIP = 2.0, -13, 46, -6


def nested_vertices(n: int, k0: int = -16) -> np.ndarray:
    s = np.power(2.0, np.arange(k0, k0 + n, dtype=np.float64))
    v = np.zeros((n, 3, 3))
    v[:, 0] = np.stack([np.zeros(n), -0.1 * s, np.full(n, -10.0)], 1)
    v[:, 1] = np.stack([np.full(n, 10.0), -0.1 * s, np.full(n, -10.0)], 1)
    v[:, 2] = np.stack([np.zeros(n), 2.0 * s, np.full(n, -10.0)], 1)
    return v


def wall_vertices(k0: int = WALL_K0, n: int = WALL_N, flip: int = WALL_FLIP, base: float = WALL_BASE) -> np.ndarray:
    v = np.zeros((n, 3, 3))
    for i in range(n):
        x = float(base) ** (k0 + i)
        if k0 + i < flip:
            v[i] = ((x, -3, -13), (x, 3, -13), (x, -3, -7))
        else:
            v[i] = ((x, 3, -7), (x, -1, -7), (x, 3, -11))
    return v


def _deep_scene(name, vertices, first=None):
    """The triangles as one mesh; with `first`, that triangle alone is a mesh of its own before the
    others (triangle 0 of batch 0, in another material: it wins every tie in t, visibly)."""
    b = S.SceneBuilder()
    if first is not None:
        b.add_mesh(*_soup_mesh(vertices[first:first + 1]), S.DRAGON_MAT, normal_interp=0)
        vertices = np.delete(vertices, first, axis=0)
    b.add_mesh(*_soup_mesh(vertices), S.BUNNY_MAT, normal_interp=0)
    return _scene(name, b)


DEEP_EVERY = 8  # ray i of a set is one of the set's own when i % DEEP_EVERY == 0


def deep_rays(cam, mode: str, seed: int) -> np.ndarray:
    """W * H T.RAY records (float32-normalized directions).  The set's own rays (deep_index) by
    mode: "inplane" (1, j * 1e-11, 0), an exact zero in z; "axis" (1, j * 1e-11, -m * 1e-11);
    "across" (dx, 0, -1) with 36 values of dx over [-0.4, 0.4], an exact zero in y.  The others go
    towards points drawn around the spheres."""
    rng = np.random.default_rng(seed)
    n = W * H
    rays = np.zeros(n, T.RAY)
    for i in range(n):
        j = i // DEEP_EVERY
        if i % DEEP_EVERY:
            target = np.array([rng.uniform(-8, 8), rng.uniform(-4, 6), rng.uniform(-20, -8)])
            d = target - np.asarray(cam, np.float64)
        elif mode == "across":
            d = np.array([-0.4 + 0.8 * (j % 36) / 35, 0.0, -1.0])
        else:
            d = np.array([1.0, (j % 5) * 1e-11, -(j % 3) * 1e-11 if mode == "axis" else 0.0])
        d = d.astype(f32)
        d = d * (f32(1) / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        rays[i]["dir"] = (*d, 1.0)
    return rays


def deep_index() -> np.ndarray:
    return np.arange(0, W * H, DEEP_EVERY)


@dataclass
class DeepSet:
    """One mesh, one camera, one ray set, and what the CPU proof asserts of it."""

    name: str
    scene: S.Scene
    rays: np.ndarray
    beyond: tuple              # walks ("binary", "wide", "quant") in which every ray of the set's own
                               # holds more entries than the walk's LDS part
    hit_tri: int | None = None  # the triangle every ray of the set's own hits, or None: they hit none
    via_tail: tuple = ()       # walks that reach hit_tri's leaf through an entry of the private tail

    def params(self, **kw):
        return self.scene.params(**kw)

    def qrays(self, idx=None) -> np.ndarray:
        """The rays (or those of `idx`) as T.QRAY records from the set's camera."""
        idx = np.arange(len(self.rays)) if idx is None else idx
        q = np.zeros(len(idx), T.QRAY)
        q["org"] = self.scene.ubo["camPos"][:3]
        q["dir"] = self.rays["dir"][idx, :3]
        return q


LDS_OF = {"binary": LDS_G2, "wide": LDS_G2, "quant": LDS_G3}


def _with_cam(sc, cam):
    return S.Scene(sc.name, S.make_ubo(cam=cam), sc.tris, sc.models, sc.env, sc.width, sc.height, sc.max_depth,
                   flags=sc.flags)


NESTED_FIRST = 4  # the nested meshes' triangle of s = 2^-12 is triangle 0 of batch 0: it wins the ties


def _deep() -> dict:
    out = {}
    binary = _deep_scene("nested136", nested_vertices(136), NESTED_FIRST)  # 4-wide bound > 64: the fallback
    wide = _deep_scene("nested100", nested_vertices(100), NESTED_FIRST)    # 4-wide bound <= 64: kept
    wall = _deep_scene("wall46", wall_vertices())
    inplane, across, miss, hit = (-1.0, 0.0, -10.0), (5.0, 0.0, 0.0), (0.0, 0.5, -9.5), (0.0, 1.5, -8.5)

    def add(name, sc, cam, mode, seed, beyond, **kw):
        out[name] = DeepSet(name, _with_cam(sc, cam), deep_rays(cam, mode, seed), beyond, **kw)

    add("binary_inplane", binary, inplane, "inplane", 1, ("binary",))
    add("binary_across", binary, across, "across", 2, ("binary",), hit_tri=0, via_tail=("binary",))
    add("wide_inplane", wide, inplane, "inplane", 3, ("wide", "quant"))
    add("wide_across", wide, across, "across", 4, ("wide", "quant"), hit_tri=0, via_tail=("wide", "quant"))
    add("wall_miss", wall, miss, "axis", 5, ("wide", "quant"))
    add("wall_hit", wall, hit, "axis", 6, ("wide", "quant"), hit_tri=WALL_FLIP - WALL_K0, via_tail=("quant",))
    return out


DEEP = _deep()
