"""Shared by tests/test_floor_lit.py and tests/test_gpu_floor_lit.py: the library's floor_lit
conditions (trt_diag_floor_lit) and a float64 host model of which floor-class tiles of a frame have
a shadow-mask bit in a lane that hits the floor (the waves that keep the shadow set-up)."""
from __future__ import annotations

import ctypes

import numpy as np

from tests.shadow_mask_common import masks
from vkcomputeshader_tinyraytracer_amd import types as T
from vkcomputeshader_tinyraytracer_amd._lib import lib

CELL = 0.25  # kShadowCellDefault


def floor_lit(flags, lights) -> int:
    """attach_floor_class's conditions on the launch's flags and lights, without the knob."""
    fn = lib().trt_diag_floor_lit
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_float)]
    lts = np.ascontiguousarray(np.asarray(lights, np.float32).reshape(9))
    return fn(int(flags), lts.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))


def floor_hits(p: T.Params, cam):
    """Float64 twin of floor_frame's floor test for every pixel of the frame: (hit[h, w], x, z)."""
    W, H = p.width, p.height
    ys, xs = np.mgrid[0:H, 0:W]
    dz = -1.0 * (H / (2.0 * np.tan(float(p.fov) / 2.0)))
    row = np.where(xs + 1 == W, ys + 1, ys) if (p.flags & T.FLAG_ROW_QUIRK) else ys
    d = np.stack([(xs + 0.5) - W * 0.5, -(row + 0.5) + H * 0.5, np.full(xs.shape, dz)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -(float(cam[1]) + 4.0) / d[..., 1]
    ok = (np.abs(d[..., 1]) > 1e-4) & (t > 1e-4) & (t < 1e10)
    t = np.where(ok, t, 0.0)
    px, pz = float(cam[0]) + d[..., 0] * t, float(cam[2]) + d[..., 2] * t
    return ok & (np.abs(px) < 10.0) & (pz < -5.0) & (pz > -30.0), px, pz


def tiles(a):
    """any() over the 8 x 8 tiles of a [h, w] mask (partial tiles padded with False)."""
    h, w = a.shape
    pad = np.zeros((-(-h // 8) * 8, -(-w // 8) * 8), bool)
    pad[:h, :w] = a
    return pad.reshape(pad.shape[0] // 8, 8, pad.shape[1] // 8, 8).any(axis=(1, 3))


def class_tiles(p: T.Params, ubo, span, sph, cells):
    """(cls, hit, dark)[tile row, tile column] of one full frame: the tile is of the floor class
    (span, sph: the frame's intervals, tests/floor_class_common.intervals), holds a floor hit,
    holds a floor hit whose mask cell has a bit set."""
    nz, nx = cells.shape
    col = np.arange((p.width + 7) // 8)[None, :]
    cls = ((col >= span[:, :1]) & (col < span[:, 1:])) & ~((col >= sph[:, :1]) & (col < sph[:, 1:]))
    hit, px, pz = floor_hits(p, np.array(ubo["camPos"][:3], np.float64))
    ix = np.clip(((px + 10.0) / CELL).astype(np.int64), 0, nx - 1)
    iz = np.clip(((pz + 30.0) / CELL).astype(np.int64), 0, nz - 1)
    return cls, tiles(hit), tiles(hit & (cells[iz, ix] != 0))


def scene_cells(ubo, flags):
    """The shadow-mask cells of a UBO's spheres and lights."""
    sph = np.array([ubo[f"sphere{i}"]["center_radius"] for i in range(4)], np.float32)
    lts = np.array([ubo[f"light{i}"][:3] for i in range(3)], np.float32)
    cells, _, fallback = masks(sph, lts, flags & T.FLAG_SPHERES, CELL)
    assert not fallback
    return cells
