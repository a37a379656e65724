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


F = np.float32
EPS = F(1e-3)
N_FLOOR = 200_000


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def query_needs(p, n, sign, sph, lts):
    """[point, light, sphere] of float32 shadow queries from hit points p with normals n, origin
    p + sign * n * EPS: (first branch passes and the chord overlaps (0, |L - p|), first branch)."""
    need = np.zeros((len(p), 3, 4), bool)
    first = np.zeros((len(p), 3, 4), bool)
    so = (p + F(sign) * n * EPS).astype(F)
    for i in range(3):
        d = (lts[i][None, :] - p).astype(F)
        dist = np.sqrt(dot(d, d)).astype(F)
        ld = (d / dist[:, None]).astype(F)
        for j in range(4):
            Lc = (sph[j, :3][None, :] - so).astype(F)
            tca = dot(Lc, ld).astype(F)
            d2 = (dot(Lc, Lc) - tca * tca).astype(F)
            r2 = F(sph[j, 3] * sph[j, 3])
            ok = d2 <= r2
            thc = np.sqrt(np.where(ok, r2 - d2, F(0))).astype(F)
            first[:, i, j] = ok
            need[:, i, j] = ok & (tca + thc > 0) & (tca - thc < dist)
    return need, first


def floor_points(sph, lts, rng, n=N_FLOOR):
    """Half uniform over the floor rectangle, half within 0.05 of a (light, sphere) shadow outline
    (the tangent cone of the sphere from the light, cut by y = -4); y perturbed by +-1e-4."""
    per = n // 2 // 12
    parts = []
    for i in range(3):
        for j in range(4):
            L, c, r = lts[i].astype(np.float64), sph[j, :3].astype(np.float64), float(sph[j, 3])
            d = c - L
            D = np.linalg.norm(d)
            if D <= r:
                continue
            centre = L + d * (1 - r * r / (D * D))
            rad = r * np.sqrt(1 - r * r / (D * D))
            u = np.cross(d, [0.0, 1.0, 0.3])
            u /= np.linalg.norm(u)
            v = np.cross(d / D, u)
            a = rng.uniform(0, 2 * np.pi, 3 * per)
            q = centre + rad * (np.cos(a)[:, None] * u + np.sin(a)[:, None] * v)
            s = (-4.0 - L[1]) / (q[:, 1] - L[1])
            pt = L + s[:, None] * (q - L)
            pt = pt[(s > 0) & np.isfinite(s)]
            pt[:, 0] += rng.uniform(-0.05, 0.05, len(pt))
            pt[:, 2] += rng.uniform(-0.05, 0.05, len(pt))
            inside = (np.abs(pt[:, 0]) < 10) & (pt[:, 2] < -5) & (pt[:, 2] > -30)
            parts.append(pt[inside][:per])
    outline = np.concatenate(parts) if parts else np.zeros((0, 3))
    nu = n - len(outline)
    uni = np.stack([rng.uniform(-10, 10, nu), np.full(nu, -4.0), rng.uniform(-30, -5, nu)], 1)
    p = np.concatenate([outline, uni])
    p[:, 1] = -4.0 + rng.uniform(-1e-4, 1e-4, len(p))
    p = p.astype(F)
    keep = (np.abs(p[:, 0]) < F(10)) & (p[:, 2] < F(-5)) & (p[:, 2] > F(-30))  # scene_intersect's test
    return p[keep], len(outline)


def cell_masks(cells, p, cell):
    nz, nx = cells.shape
    inv = F(1.0 / cell)
    ix = np.clip(((p[:, 0] + F(10)) * inv).astype(np.int32), 0, nx - 1)
    iz = np.clip(((p[:, 2] + F(30)) * inv).astype(np.int32), 0, nz - 1)
    return cells[iz, ix].astype(np.uint32)


def bits(m):
    """[..., light, sphere] booleans of masks."""
    return ((np.asarray(m)[..., None] >> np.arange(12)) & 1).astype(bool).reshape(*np.shape(m), 3, 4)
