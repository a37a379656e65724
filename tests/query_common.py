"""Shared by tests/test_gpu_query.py and tests/test_gpu_random_scenes.py: ray sets for
Renderer.trace_rays and what the CPU oracle says of them (colours and counters through its
cast_ray, hit records built in the shader's own order from its single-ray probes).  No GPU."""
from __future__ import annotations

import ctypes

import numpy as np

from oracle import oracle as orc
from vkcomputeshader_tinyraytracer_amd import types as T

f32 = np.float32
EPS = f32(0.0001)  # MIN_EPSILON, shader.comp:78


def fa(v):
    return (ctypes.c_float * len(v))(*[float(x) for x in v])


def normalize32(v):
    """The shader's normalize in float32 numpy: v * (1 / sqrt((x x + y y) + z z))."""
    v = np.asarray(v, f32)
    inv = f32(1) / np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    return v * inv[..., None]


def random_rays(n: int, seed: int) -> np.ndarray:
    """Origins uniform in x [-8, 8], y [-3, 6], z [-28, 2] (inside the spheres and the mesh
    included); directions uniform on the sphere times a length in [0.1, 10]."""
    rng = np.random.default_rng(seed)
    q = np.zeros(n, T.QRAY)
    q["org"] = rng.uniform((-8, -3, -28), (8, 6, 2), size=(n, 3)).astype(f32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    q["dir"] = (d * rng.uniform(0.1, 10.0, size=(n, 1))).astype(f32)
    return q


def oracle_colours(b, p, rays):
    """Per ray: the oracle's cast_ray from the ray's origin along the float32-normalized direction;
    its clamped linear colour through the shader's gamma and pack.  Returns (rgba8, rgba32f, summed
    counters)."""
    L = orc.lib()
    d = normalize32(rays["dir"])
    n = len(rays)
    lin = np.zeros((n, 3), f32)
    tot = {k: 0 for k in T.Stats.EXACT_WALK}
    out = (ctypes.c_float * 3)()
    st = T.Stats()
    for i in range(n):
        L.orc_cast_ray(ctypes.byref(b.s), ctypes.byref(p), orc.MODE_FAST, fa(rays["org"][i]), fa(d[i]), out,
                       ctypes.byref(st))
        lin[i] = out[:]
        for k in tot:
            tot[k] += int(getattr(st, k))
    g = np.power(lin, f32(2.2)).astype(f32)
    ref32 = np.concatenate([g, np.ones((n, 1), f32)], 1)
    ref8 = np.concatenate([np.floor(f32(255) * g + f32(0.5)).astype(np.uint8), np.full((n, 1), 255, np.uint8)], 1)
    return ref8, ref32, tot


def expected_hits(sc, rays):
    """scene_intersect in the shader's own order with a strict `<` throughout: the floor
    (shader.comp:302-320 restated in float32 numpy), the spheres 0..3 (orc_ray_sphere), then every
    batch in order behind orc_ray_aabb with orc_ray_triangle over its triangles."""
    L = orc.lib()
    spheres = [np.asarray(sc.ubo[f"sphere{i}"]["center_radius"], f32) for i in range(4)]
    sph_c = [fa(s) for s in spheres]
    tri_c = [[fa(sc.tris[k][j][:3]) for k in ("v0", "v1", "v2", "v0_norm", "v1_norm", "v2_norm")] for j in range(len(sc.tris))]
    boxes = [(fa(m["bboxMin"][:3]), fa(m["bboxMax"][:3]), int(m["params0"][0]), int(m["params0"][1]), int(m["params0"][2]))
             for m in sc.models]
    dirs = normalize32(rays["dir"])
    out = np.zeros(len(rays), T.QHIT)
    t = ctypes.c_float(0)
    nrm = (ctypes.c_float * 3)()
    for i in range(len(rays)):
        o, d = rays["org"][i], dirs[i]
        oc, dc = fa(o), fa(d)
        best, kind, idx, n = f32(1e10), T.HIT_NONE, 0, np.zeros(3, f32)
        if sc.flags & T.FLAG_FLOOR and abs(d[1]) > EPS:
            tf = -(o[1] + f32(4.0)) / d[1]
            if tf > EPS and tf < best:
                pt = o + d * tf
                if abs(pt[0]) < f32(10.0) and pt[2] < f32(-5.0) and pt[2] > f32(-30.0):
                    best, kind, n = tf, T.HIT_FLOOR, np.array((0, 1, 0), f32)
        if sc.flags & T.FLAG_SPHERES:
            for s in range(4):
                if L.orc_ray_sphere(oc, dc, sph_c[s], ctypes.byref(t)) and f32(t.value) < best:
                    best, kind, idx = f32(t.value), T.HIT_SPHERE, s
                    n = normalize32((o + d * best) - spheres[s][:3])
        for bmin, bmax, start, count, ni in boxes:
            if not L.orc_ray_aabb(oc, dc, bmin, bmax):
                continue
            for j in range(start, start + count):
                if L.orc_ray_triangle(oc, dc, *tri_c[j], ni, ctypes.byref(t), nrm) and f32(t.value) > EPS and f32(t.value) < best:
                    best, kind, idx, n = f32(t.value), T.HIT_TRIANGLE, j, np.array(nrm[:], f32)
        out[i]["t"], out[i]["kind"], out[i]["index"], out[i]["n"] = best, kind, idx, n
    return out
