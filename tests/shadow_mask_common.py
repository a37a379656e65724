"""Shared by tests/test_shadow_mask.py and tests/test_gpu_shadow_mask.py: the shadow occluder
masks of a UBO through the library's diagnostic entry (trt_diag_shadow_mask, no GPU), and the
scenes both files use."""
from __future__ import annotations

import ctypes

import numpy as np

from vkcomputeshader_tinyraytracer_amd import scene as S, types as T
from vkcomputeshader_tinyraytracer_amd._lib import lib

ALL = 0x0FFF
REF_SPHERES = np.array([s[0] for s in S.SPHERES], np.float32)
REF_LIGHTS = np.array(S.LIGHTS, np.float32)


def masks(spheres, lights, flags=T.FLAG_SPHERES | T.FLAG_FLOOR, cell=0.25):
    """(cells[nz, nx], rows[4], fallback) of 4 x (centre, radius) spheres and 3 lights."""
    sph = np.ascontiguousarray(np.asarray(spheres, np.float32).reshape(16))
    lts = np.ascontiguousarray(np.asarray(lights, np.float32).reshape(9))
    cap = 200 * 250
    out = np.zeros(cap, np.uint16)
    rows = np.zeros(4, np.uint32)
    nx, nz = ctypes.c_uint32(0), ctypes.c_uint32(0)
    fp, up = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    rc = lib().trt_diag_shadow_mask(sph.ctypes.data_as(fp), lts.ctypes.data_as(fp), int(flags), float(cell),
                                    out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), cap, ctypes.byref(nx),
                                    ctypes.byref(nz), rows.ctypes.data_as(up))
    assert rc in (0, 1), rc
    return out[: nx.value * nz.value].reshape(nz.value, nx.value).copy(), rows, bool(rc)


def seeded_scene(seed: int):
    """Moved spheres and lights: centres over the floor, radii 0.5..4, lights well outside."""
    rng = np.random.default_rng(seed)
    sph = np.stack([rng.uniform(-8, 8, 4), rng.uniform(-3, 6, 4), rng.uniform(-28, -7, 4), rng.uniform(0.5, 4, 4)], 1)
    ang = rng.uniform(0, 2 * np.pi, 3)
    rad = rng.uniform(25, 60, 3)
    lts = np.stack([rad * np.cos(ang), rng.uniform(15, 50, 3), -17 + rad * np.sin(ang)], 1)
    return sph.astype(np.float32), lts.astype(np.float32)


def cutting_floor_scene():
    sph = REF_SPHERES.copy()
    sph[1] = (-1.0, -4.5, -12.0, 2.0)  # cuts the plane y = -4
    return sph, REF_LIGHTS.copy()


def overlapping_scene():
    sph = REF_SPHERES.copy()
    sph[2] = (-2.0, 0.5, -15.0, 3.0)  # overlaps sphere 0 at (-3, 0, -16), r 2
    return sph, REF_LIGHTS.copy()


def ubo_with(ubo, spheres=None, lights=None):
    u = np.array(ubo, dtype=T.UBO)  # a 0-d copy, also of an element of a UBO array
    if spheres is not None:
        for i in range(4):
            u[f"sphere{i}"]["center_radius"] = tuple(float(v) for v in spheres[i])
    if lights is not None:
        for i in range(3):
            u[f"light{i}"][:3] = np.asarray(lights[i], np.float32)
    return u
