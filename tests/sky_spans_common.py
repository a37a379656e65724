"""Shared by tests/test_sky_spans.py and tests/test_gpu_sky_spans.py: the span tables of a launch
through the library's diagnostic entry, and the cameras both files try to break them with."""
from __future__ import annotations

import copy
import ctypes

import numpy as np

from oracle import oracle as orc
from vkcomputeshader_tinyraytracer_amd import scene as S, types as T
from vkcomputeshader_tinyraytracer_amd._lib import lib

GLASS_C, GLASS_R = (-1.0, -1.5, -12.0), 2.0  # scene.SPHERES[1]

# name -> camera positions of one group (one launch)
ADVERSARIAL = {
    "glass_centre": [GLASS_C],
    "glass_surface": [(GLASS_C[0], GLASS_C[1], GLASS_C[2] + GLASS_R)],
    "glass_just_outside": [(GLASS_C[0], GLASS_C[1], GLASS_C[2] + GLASS_R + 1e-3)],
    "below_floor": [(0.0, -6.0, 0.0)],
    "on_floor": [(0.0, -4.0, 0.0)],
    "just_above_floor": [(0.0, -4.0 + 1e-5, 0.0)],
    "far_back": [(0.0, 0.0, 1000.0)],
    "scene_behind": [(0.0, 0.0, -100.0)],
    "fifty_apart": [(0.0, 0.0, 0.0), (50.0, 0.0, 0.0)],
}
NON_FINITE = [(float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 0.0, float("-inf"))]
# the fallbacks of the construction: every row full
MUST_BE_FULL = ("glass_centre", "glass_surface", "below_floor", "on_floor", "just_above_floor", "fifty_apart")


def at(sc, ubo):
    s = copy.copy(sc)
    s.ubo = ubo
    return s


def ubos_at(ubo, cams):
    out = np.repeat(ubo[None], len(cams), axis=0).copy()
    for k, c in enumerate(cams):
        out[k]["camPos"][:3] = np.array(c, np.float32)
    return out


def spans(p: T.Params, ubos, group_frames: int = 16, rays_in: bool = False) -> np.ndarray:
    """The launch's span tables as an int array [frame, tile row, (c0, c1)], expanded per frame;
    a launch that runs with spans off has every row full."""
    n = len(ubos)
    sph = np.array([ubos[0][f"sphere{i}"]["center_radius"] for i in range(4)], np.float32).reshape(16)
    cams = np.ascontiguousarray(np.array([u["camPos"][:3] for u in ubos], np.float32).reshape(-1))
    cap = 4096
    out = np.zeros(cap, np.uint32)
    ntr, shift = ctypes.c_uint32(0), ctypes.c_uint32(0)
    fn = lib().trt_diag_sky_spans
    fn.restype = ctypes.c_int
    u32, fp, up = ctypes.c_uint32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    fn.argtypes = [u32, u32, ctypes.c_float, u32, u32, u32, u32, ctypes.c_int, fp, fp, u32, u32, up, u32, up, up]
    tabs = fn(p.width, p.height, p.fov, p.flags, p.band_rows, p.band_count, p.band_index, int(rays_in),
              sph.ctypes.data_as(fp), cams.ctypes.data_as(fp), n, group_frames, out.ctypes.data_as(up), cap,
              ctypes.byref(ntr), ctypes.byref(shift))
    assert tabs >= 0
    ntx = (p.width + 7) // 8
    rows = len(T.output_rows(p.height, p.band_rows, p.band_count, p.band_index))
    if tabs == 0:
        full = np.zeros((n, (rows + 7) // 8, 2), np.int64)
        full[..., 1] = ntx
        return full
    assert ntr.value == (rows + 7) // 8 and shift.value >= 1 and tabs == -(-n // (1 << shift.value))
    w = out[: tabs * ntr.value].reshape(tabs, ntr.value).astype(np.int64)
    tab = np.stack([w & 0xFFFF, np.minimum(w >> 16, ntx)], axis=-1)
    assert (tab[..., 0] <= tab[..., 1]).all()
    return tab[np.arange(n) >> shift.value]


def is_full(span: np.ndarray, width: int) -> bool:
    return bool((span[..., 0] == 0).all() and (span[..., 1] == (width + 7) // 8).all())


def culled_share(span: np.ndarray, width: int) -> float:
    """Share of the launch's tile-frames outside the spans."""
    ntx = (width + 7) // 8
    return 1.0 - float((span[..., 1] - span[..., 0]).sum()) / (span.shape[0] * span.shape[1] * ntx)


_BG: dict = {}


def background() -> np.ndarray:
    """The RGBA8 the oracle writes for a primary miss with the envmap off."""
    if "bg" not in _BG:
        small = S.config_c2(16, 8, env_size=(64, 32))
        _BG["bg"] = orc.render(small, small.params(max_depth=1, flags=T.FLAG_ROW_QUIRK))[0][0, 0]
    return _BG["bg"]


def hits(sc, ubo, flags=None, **params):
    """Per-pixel primary hit mask as tests/test_gpu_sky_table.py::_oracle derives it: the oracle's
    depth-1 frame with the envmap off, compared with the constant background.  `params`: further
    settings of the frame (fov)."""
    a = at(sc, ubo)
    fl = (sc.flags if flags is None else flags) & ~T.FLAG_ENVMAP
    m8 = orc.render(a, a.params(max_depth=1, flags=fl, **params))[0]
    return ~(m8 == background()).all(axis=-1)


def assert_inside(hits, span, rows=None, what="hit pixels outside their span"):
    """Every hit pixel of frame rows `rows` (all, or a band group's) lies inside its row's span."""
    if rows is not None:
        hits = hits[rows]
    ys, xs = np.nonzero(hits)
    c0, c1 = span[ys // 8, 0], span[ys // 8, 1]
    bad = (xs // 8 < c0) | (xs // 8 >= c1)
    assert not bad.any(), f"{int(bad.sum())} {what}, first at compact row {ys[bad][0]}, x {xs[bad][0]}"
