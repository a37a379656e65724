"""Shared by tests/test_occlusion_host.py and tests/test_gpu_occlusion.py: what the CPU oracle says
of an occlusion query (abi.h trt_occluded), and segment sets around a ray set's own hit distances.
No GPU.

The contract is occluded(org, dir, tmax) == (hit.t < tmax), hit = scene_intersect's record of the
ray: the reference is tests/query_common.expected_hits, the shader-order restatement over the
oracle's single-ray probes, with the floor test on or off as the query's flags say."""
from __future__ import annotations

import copy

import numpy as np

from tests.query_common import expected_hits, f32
from vkcomputeshader_tinyraytracer_amd import scene as S, types as T

INF32 = f32(np.inf)


def _with_floor(sc, flags: int):
    """`sc` with its floor flag as `flags` has it (expected_hits reads sc.flags)."""
    want = (int(sc.flags) & ~T.FLAG_FLOOR) | (int(flags) & T.FLAG_FLOOR)
    if want == int(sc.flags):
        return sc
    other = copy.copy(sc)
    other.flags = want
    return other


def rays_of(segs: np.ndarray) -> np.ndarray:
    r = np.zeros(segs.shape, T.QRAY)
    r["org"], r["dir"] = segs["org"], segs["dir"]
    return r


def expected_occluded(sc, segs: np.ndarray, flags: int, hits: np.ndarray | None = None) -> np.ndarray:
    """(n,) uint8 of T.OCC_OCCLUDED / T.OCC_VISIBLE: hits.t < tmax in float32, hits = expected_hits of
    the segments' rays in `sc` with the floor as `flags` says.  `hits`, when given, are those
    records computed before (one per segment, same floor flag): a reference is computed once."""
    segs = np.ascontiguousarray(segs, T.QSEG).reshape(-1)
    if hits is None:
        hits = expected_hits(_with_floor(sc, flags), rays_of(segs))
    assert len(hits) == len(segs)
    occ = hits["t"].astype(f32) < segs["tmax"].astype(f32)
    return np.where(occ, T.OCC_OCCLUDED, T.OCC_VISIBLE).astype(np.uint8)


def hits_for(sc, rays: np.ndarray, flags: int) -> np.ndarray:
    """expected_hits of `rays` with the floor as `flags` says."""
    return expected_hits(_with_floor(sc, flags), rays)


def hits_without_floor(sc, rays: np.ndarray, hits_on: np.ndarray) -> np.ndarray:
    """hits_for(sc, rays, no floor) from the records with the floor: the floor test is
    scene_intersect's first and only ever lowers the nearest distance, so a ray whose nearest hit is
    not the floor keeps its record; only the floor's rays are traced again."""
    out = hits_on.copy()
    fl = np.flatnonzero(hits_on["kind"] == T.HIT_FLOOR)
    if len(fl):
        out[fl] = hits_for(sc, rays[fl], int(sc.flags) & ~T.FLAG_FLOOR)
    return out


def boundary_segments(rays: np.ndarray, hits: np.ndarray):
    """Around each ray's own hit distance t: three segments per hit, tmax = t (visible: the test is
    strict), nextafter(t, +inf) (occluded) and 0.5 t (whatever the reference says: no nearer surface
    exists); one per miss, tmax = 1e10 (visible).  Returns (segs, ray index of each segment)."""
    idx, tm = [], []
    for i, h in enumerate(hits):
        t = f32(h["t"])
        if h["kind"] == T.HIT_NONE:
            idx.append(i)
            tm.append(T.QSEG_MAX_T)
        else:
            idx += [i, i, i]
            tm += [t, np.nextafter(t, INF32), f32(0.5) * t]
    idx = np.asarray(idx)
    return S.segments_from_rays(rays[idx], np.asarray(tm, f32)), idx
