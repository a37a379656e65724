"""Shared by tests/test_sphere_spans.py and tests/test_gpu_floor_class.py: the raw span words and
sphere-interval words of a launch through the library's diagnostic entries, the relation the two
must keep, and the floor class they define (tiles inside the span and outside the interval)."""
from __future__ import annotations

import ctypes

import numpy as np

from oracle import oracle as orc
from tests.sky_spans_common import assert_inside, at, background
from vkcomputeshader_tinyraytracer_amd import types as T
from vkcomputeshader_tinyraytracer_amd._lib import lib

SPAN_FULL = 0xFFFF0000


def raw_words(entry: str, p: T.Params, ubos, group_frames: int = 16, rays_in: bool = False):
    """(tables, shift, words[tables, tile rows]) of `entry` (trt_diag_sky_spans or
    trt_diag_sphere_spans); tables == 0: spans off for this launch."""
    n = len(ubos)
    sph = np.array([ubos[0][f"sphere{i}"]["center_radius"] for i in range(4)], np.float32).reshape(16)
    cams = np.ascontiguousarray(np.array([u["camPos"][:3] for u in ubos], np.float32).reshape(-1))
    cap = 4096
    out = np.zeros(cap, np.uint32)
    ntr, shift = ctypes.c_uint32(0), ctypes.c_uint32(0)
    fn = getattr(lib(), entry)
    fn.restype = ctypes.c_int
    u32, fp, up = ctypes.c_uint32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    fn.argtypes = [u32, u32, ctypes.c_float, u32, u32, u32, u32, ctypes.c_int, fp, fp, u32, u32, up, u32, up, up]
    tabs = fn(p.width, p.height, p.fov, p.flags, p.band_rows, p.band_count, p.band_index, int(rays_in),
              sph.ctypes.data_as(fp), cams.ctypes.data_as(fp), n, group_frames, out.ctypes.data_as(up), cap,
              ctypes.byref(ntr), ctypes.byref(shift))
    assert tabs >= 0
    return tabs, shift.value, out[: tabs * ntr.value].reshape(tabs, ntr.value).copy()


def intervals(p: T.Params, ubos, group_frames: int = 16, rays_in: bool = False):
    """(span, sph): int arrays [frame, tile row, (lo, hi)] of tile columns, expanded per frame, after
    checking the relation of the two on the raw words; None when the launch runs with spans off
    (the floor class is then off too)."""
    tabs, shift, w = raw_words("trt_diag_sky_spans", p, ubos, group_frames, rays_in)
    stabs, sshift, s = raw_words("trt_diag_sphere_spans", p, ubos, group_frames, rays_in)
    assert (tabs, shift, w.shape) == (stabs, sshift, s.shape)
    if tabs == 0:
        return None
    ntx = (p.width + 7) // 8
    full = w == SPAN_FULL
    assert (s[full] == SPAN_FULL).all(), "a full span with a sphere interval that is not full"
    if not (p.flags & T.FLAG_SPHERES):
        assert (s[~full] == 0).all(), "spheres off: the interval must be empty"
    w, s = w.astype(np.int64), s.astype(np.int64)
    span = np.stack([w & 0xFFFF, np.minimum(w >> 16, ntx)], axis=-1)
    sph = np.stack([s & 0xFFFF, np.minimum(s >> 16, ntx)], axis=-1)
    assert (span[..., 0] <= span[..., 1]).all() and (sph[..., 0] <= sph[..., 1]).all()
    ne = (sph[..., 1] > sph[..., 0]) & ~full  # a non-empty interval lies inside its span
    assert (sph[..., 0][ne] >= span[..., 0][ne]).all() and (sph[..., 1][ne] <= span[..., 1][ne]).all()
    f = np.arange(len(ubos)) >> shift
    return span[f], sph[f]


def floor_tiles(span: np.ndarray, sph: np.ndarray) -> int:
    """Tile-frames of the floor class: inside the span, outside the sphere interval."""
    inside = span[..., 1] - span[..., 0]
    both = np.maximum(0, np.minimum(span[..., 1], sph[..., 1]) - np.maximum(span[..., 0], sph[..., 0]))
    return int((inside - both).sum())


def floor_share(span: np.ndarray, sph: np.ndarray, width: int) -> float:
    return floor_tiles(span, sph) / (span.shape[0] * span.shape[1] * ((width + 7) // 8))


def sphere_hits(sc, ubo, flags=None, **params):
    """Per-pixel mask of the primary rays that hit a sphere with the floor out of the way (every
    ray that passes sphere_hit, also one whose floor hit is nearer): the oracle's depth-1 frame
    without envmap and floor, compared with the constant background.  Spheres off: none.
    `params`: further settings of the frame (fov)."""
    fl = sc.flags if flags is None else flags
    if not (fl & T.FLAG_SPHERES):
        return np.zeros((sc.height, sc.width), bool)
    a = at(sc, ubo)
    m8 = orc.render(a, a.params(max_depth=1, flags=fl & ~T.FLAG_ENVMAP & ~T.FLAG_FLOOR, **params))[0]
    return ~(m8 == background()).all(axis=-1)


def assert_inside_interval(hits, sph, rows=None):
    assert_inside(hits, sph, rows, what="sphere pixels outside their interval")
