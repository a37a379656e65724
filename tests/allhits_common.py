"""Shared by tests/test_allhits_host.py and tests/test_gpu_allhits.py: what the CPU oracle says of an
all-hits query (abi.h trt_trace_all).  No GPU.

The reference is built like tests/query_common.expected_hits, from the oracle's single-ray probes:
every candidate of a segment (the floor restated in float32 numpy, both roots of every sphere
restated in float32 in the kernel's term order, orc_ray_aabb per batch and orc_ray_triangle over its
triangles), each kept iff MIN_EPSILON < t < tmax, sorted by the key (t, class, a, b).  On every
segment it asserts that the restated nearer sphere root is orc_ray_sphere's t and that record 0 is
expected_hits' record."""
from __future__ import annotations

import copy
import ctypes

import numpy as np

from oracle import oracle as orc
from tests.query_common import EPS, expected_hits, f32, fa, normalize32
from vkcomputeshader_tinyraytracer_amd import types as T

MASK = T.FLAG_FLOOR | T.FLAG_SPHERES
MISS = np.zeros(1, T.QHIT)
MISS["t"] = f32(1e10)


def with_flags(sc, flags: int):
    """`sc` with its floor and sphere flags as `flags` has them (expected_hits reads sc.flags)."""
    want = (int(sc.flags) & ~MASK) | (int(flags) & MASK)
    if want == int(sc.flags):
        return sc
    other = copy.copy(sc)
    other.flags = want
    return other


def rays_of(segs: np.ndarray) -> np.ndarray:
    r = np.zeros(segs.shape, T.QRAY)
    r["org"], r["dir"] = segs["org"], segs["dir"]
    return r


def sphere_roots(o, d, cr):
    """ray_sphere_intersect's terms in float32, every product and sum rounded on its own in the dot
    order (x x + y y) + z z, the square root correctly rounded: (t0, t1), or None when the ray passes
    the sphere by (d2 > r2; a NaN goes on, as in the shader, and then fails every comparison)."""
    L = cr[:3] - o
    tca = (L[0] * d[0] + L[1] * d[1]) + L[2] * d[2]
    d2 = ((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2]) - tca * tca
    r2 = cr[3] * cr[3]
    if d2 > r2:
        return None
    with np.errstate(invalid="ignore"):
        thc = np.sqrt(r2 - d2, dtype=f32)
    return f32(tca - thc), f32(tca + thc)


def all_candidates(sc, segs: np.ndarray, flags: int, first: np.ndarray | None = None) -> list:
    """Per segment the sorted list of (t, class, a, b, kind, index, n) of every hit inside (MIN_EPSILON,
    tmax).  `first`, when given, are expected_hits' records of the segments' rays under the same
    flags, computed before."""
    segs = np.ascontiguousarray(segs, T.QSEG).reshape(-1)
    L = orc.lib()
    spheres = [np.asarray(sc.ubo[f"sphere{i}"]["center_radius"], f32).reshape(4) for i in range(4)]
    sph_c = [fa(s) for s in spheres]
    tri_c = [[fa(sc.tris[k][j][:3]) for k in ("v0", "v1", "v2", "v0_norm", "v1_norm", "v2_norm")] for j in range(len(sc.tris))]
    boxes = [(fa(m["bboxMin"][:3]), fa(m["bboxMax"][:3]), int(m["params0"][0]), int(m["params0"][1]), int(m["params0"][2]))
             for m in sc.models]
    if first is None:
        first = expected_hits(with_flags(sc, flags), rays_of(segs))
    assert len(first) == len(segs)
    dirs = normalize32(segs["dir"])
    t = ctypes.c_float(0)
    nrm = (ctypes.c_float * 3)()
    out = []
    for i in range(len(segs)):
        o, d, tmax = segs["org"][i], dirs[i], f32(segs["tmax"][i])
        oc, dc = fa(o), fa(d)
        c = []
        if flags & T.FLAG_FLOOR and abs(d[1]) > EPS:
            tf = -(o[1] + f32(4.0)) / d[1]
            if tf > EPS and tf < tmax:
                pt = o + d * tf
                if abs(pt[0]) < f32(10.0) and pt[2] < f32(-5.0) and pt[2] > f32(-30.0):
                    c.append((f32(tf), 0, 0, 0, T.HIT_FLOOR, 0, np.array((0, 1, 0), f32)))
        if flags & T.FLAG_SPHERES:
            for s in range(4):
                roots = sphere_roots(o, d, spheres[s])
                kept = []
                if roots is not None:
                    t0, t1 = roots
                    if t0 > EPS:
                        kept.append(t0)
                    if t1 > EPS and not (kept and t1 == kept[0]):
                        kept.append(t1)
                hit = L.orc_ray_sphere(oc, dc, sph_c[s], ctypes.byref(t))
                assert bool(hit) == bool(kept), (i, s, roots)
                if kept:
                    assert kept[0].tobytes() == f32(t.value).tobytes(), (i, s, kept, t.value)
                for tr in kept:
                    if tr < tmax:
                        c.append((tr, 1, s, 0, T.HIT_SPHERE, s, normalize32((o + d * tr) - spheres[s][:3])))
        for b, (bmin, bmax, start, count, ni) in enumerate(boxes):
            if not L.orc_ray_aabb(oc, dc, bmin, bmax):
                continue
            for j in range(start, start + count):
                if L.orc_ray_triangle(oc, dc, *tri_c[j], ni, ctypes.byref(t), nrm) and f32(t.value) > EPS and f32(t.value) < tmax:
                    c.append((f32(t.value), 2, b, j, T.HIT_TRIANGLE, j, np.array(nrm[:], f32)))
        c.sort(key=lambda r: r[:4])
        h = first[i]
        if f32(h["t"]) < tmax:
            assert c and h["kind"] != T.HIT_NONE, (i, h)
            assert (c[0][0].tobytes(), c[0][4], c[0][5]) == (f32(h["t"]).tobytes(), int(h["kind"]), int(h["index"])), (i, c[0], h)
            assert c[0][6].tobytes() == np.asarray(h["n"], f32).tobytes(), (i, c[0], h)
        else:
            assert not c, (i, c[0], h)
        out.append(c)
    return out


def records(cands: list, max_hits: int):
    """(hits (n, max_hits) T.QHIT with u = v = 0, counts (n,) uint32) of all_candidates' lists."""
    hits = np.tile(MISS, (len(cands), max_hits))
    counts = np.zeros(len(cands), np.uint32)
    for i, c in enumerate(cands):
        m = min(len(c), max_hits)
        for j in range(m):
            hits[i, j]["t"], hits[i, j]["kind"], hits[i, j]["index"], hits[i, j]["n"] = c[j][0], c[j][4], c[j][5], c[j][6]
        counts[i] = m | (T.ALLHITS_MORE if len(c) > max_hits else 0)
    return hits, counts


def expected_all_hits(sc, segs: np.ndarray, flags: int, max_hits: int, cands: list | None = None):
    """The reference answer of trt_trace_all: (hits, counts); u and v of the records are 0 (the tests
    check them by the barycentric point).  `cands`: all_candidates of the same query, computed before."""
    if cands is None:
        cands = all_candidates(sc, segs, flags)
    return records(cands, max_hits)


def totals(cands: list) -> np.ndarray:
    return np.array([len(c) for c in cands])


def equal_t_pairs(cands: list) -> int:
    """Neighbouring records of one segment with the same t."""
    return sum(1 for c in cands for a, b in zip(c, c[1:]) if a[0] == b[0])


def same_records(got: np.ndarray, want: np.ndarray):
    """t, kind, index and n of every slot, byte for byte."""
    for k in ("t", "kind", "index", "n"):
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
