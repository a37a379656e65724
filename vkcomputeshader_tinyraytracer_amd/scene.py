"""Scenes: the reference's config.hpp / main.cpp scene description, the benchmark
configurations C1-C5 (BASELINE.json), and seeded synthetic inputs (envmaps, icospheres).

Reference sources mirrored here:
  * sphere materials, spheres and lights  main.cpp:125-143
  * UBO fill                              main.cpp:2165-2179 (bboxMin/Max sentinels :120-121)
  * mesh materials / transforms / list    config.hpp:10-101 (ModelInfo: geometry.hpp:48-70)
Meshes are turned into Triangle/Model records by the product's C++ scene builder
(libtrt: trt_scene_add_mesh / trt_scene_add_obj), i.e. the same code path a C++ host uses.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from . import types as T
from ._lib import TrtError, lib

FLT_MAX = np.float32(3.402823466e38)


def material(albedo, diffuse_specular, refractive) -> np.ndarray:
    m = np.zeros((), T.MATERIAL)
    m["albedo"] = albedo
    m["diffuse_specular"] = diffuse_specular
    m["refractive"] = refractive
    return m


# main.cpp:125-128
IVORY = material((0.9, 0.5, 0.1, 0.0), (0.4, 0.4, 0.3, 50.0), (1.0, 0.0, 0.0, 0.0))
GLASS = material((0.0, 0.9, 0.1, 0.8), (0.6, 0.7, 0.8, 125.0), (1.5, 0.0, 0.0, 0.0))
RED_RUBBER = material((1.4, 0.3, 0.0, 0.0), (0.3, 0.1, 0.1, 10.0), (1.0, 0.0, 0.0, 0.0))
MIRROR = material((0.0, 16.0, 0.8, 0.0), (1.0, 1.0, 1.0, 1425.0), (1.0, 0.0, 0.0, 0.0))

# main.cpp:132-137
SPHERES = (
    ((-3.0, 0.0, -16.0, 2.0), IVORY),
    ((-1.0, -1.5, -12.0, 2.0), GLASS),
    ((1.5, -0.5, -18.0, 3.0), RED_RUBBER),
    ((7.0, 5.0, -18.0, 4.0), MIRROR),
)
# main.cpp:139-143
LIGHTS = ((-20.0, 20.0, 20.0), (30.0, 50.0, -25.0), (30.0, 20.0, 30.0))

# config.hpp:10-81 mesh materials
DUCK_MAT = material((0.0, 0.5, 0.1, 0.8), (0.6, 0.7, 0.8, 125.0), (1.5, 0.0, 0.0, 0.0))
ASSCHERCUT_MAT = material((0.0, 0.5, 0.1, 0.8), (0.6, 0.7, 0.8, 125.0), (1.5, 0.0, 0.0, 0.0))
BUNNY_MAT = material((0.9, 0.5, 0.0, 0.0), (0.0522876, 0.156863, 0.117647, 10.0), (1.0, 0.0, 0.0, 0.0))
DRAGON_MAT = material((0.9, 0.1, 0.0, 0.0), (0.013072, 0.078431, 0.143791, 10.0), (1.0, 0.0, 0.0, 0.0))
VENUS_MAT = material((0.0, 10.0, 0.8, 0.0), (1.0, 1.0, 1.0, 1425.0), (1.0, 0.0, 0.0, 0.0))
FUDANLOGO_MAT = material((0.7, 0.7, 0.0, 0.0), (0.515625, 0.3984275, 0.32421875, 12.0), (1.0, 0.0, 0.0, 0.0))
GLASS_MESH_MAT = material((0.0, 0.3, 0.05, 0.9), (0.95, 0.95, 0.95, 80.0), (1.5, 0.0, 0.0, 0.0))
WHISKY_MAT = material((0.3, 0.4, 0.05, 0.7), (0.9, 0.6, 0.3, 20.0), (1.2, 0.0, 0.0, 0.0))
ICE_MAT = material((0.05, 0.4, 0.2, 0.8), (0.8, 0.85, 0.9, 20.0), (1.31, 0.0, 0.0, 0.0))


@dataclass(frozen=True)
class ModelInfo:
    """geometry.hpp:48-70 ModelInfo + Model(material, normalinterpolation)."""

    asset: str  # file name under VCSA/assets (reference) / key in the golden mesh bundle
    material: np.ndarray
    scale: tuple
    rotation: tuple  # degrees
    translation: tuple
    normal_interp: int


# config.hpp:10-93
MODEL_INFOS = {
    "duck": ModelInfo("duck.obj", DUCK_MAT, (1, 1, 1), (0, 0, 0), (0, 0, 0), 1),
    "asschercut": ModelInfo("asschercut-mesh.obj", ASSCHERCUT_MAT, (2, 2, 2), (45, 45, 0), (0.2, -2.0, -14.0), 0),
    "bunny": ModelInfo("bunny-mesh.obj", BUNNY_MAT, (1, 1, 1), (0, 0, 0), (2.5, -1.5, -5.5), 0),
    "dragon": ModelInfo("dragon-mesh.obj", DRAGON_MAT, (0.7, 0.7, 0.7), (0, 110, 0), (-2.5, -2.175, -4.45), 1),
    "venus": ModelInfo("venus-mesh.obj", VENUS_MAT, (5.5, 5.5, 5.5), (0, 0, 0), (-1.0, 2.0, -19.0), 1),
    "fudanlogo": ModelInfo("fudanlogo-mesh.obj", FUDANLOGO_MAT, (0.4, 0.4, 0.4), (90, 0, 0), (0.85, 1.95, -4.15), 0),
    "glass": ModelInfo("glass.obj", GLASS_MESH_MAT, (1, 1, 1), (0, 0, 0), (0.0, -2.0, -8.0), 1),
    "water": ModelInfo("water.obj", WHISKY_MAT, (1, 1, 1), (0, 0, 0), (0.0, -2.0, -8.0), 1),
    "ice": ModelInfo("ice.obj", ICE_MAT, (1, 1, 1), (0, 0, 0), (0.0, -2.0, -8.0), 1),
}
DEFAULT_MODEL_LIST = ("glass", "water", "ice")  # config.hpp:97-101
README_MODEL_LIST = ("asschercut", "bunny", "dragon", "venus", "fudanlogo")  # config.hpp:96


def make_ubo(cam=(0.0, 0.0, 0.0), spheres=SPHERES, lights=LIGHTS) -> np.ndarray:
    """updateUniformBuffer (main.cpp:2165-2179)."""
    u = np.zeros((), T.UBO)
    for i, (cr, mat) in enumerate(spheres):
        u[f"sphere{i}"]["center_radius"] = cr
        u[f"sphere{i}"]["material"] = mat
    for i, l in enumerate(lights):
        u[f"light{i}"] = (*l, 1.0)
    u["camPos"] = (*cam, 1.0)
    u["bboxMin"] = FLT_MAX
    u["bboxMax"] = -FLT_MAX
    return u


def camera_path(ubo: np.ndarray, n: int, speed: float = 0.02) -> np.ndarray:
    """n per-frame UBOs of the reference's interactive loop with W and D held: processInput
    (main.cpp:391-403) moves cameraPos by cameraSpeed along cameraFront (0, 0, -1) and along
    normalize(cross(cameraFront, cameraUp)) = (1, 0, 0) every frame, and updateUniformBuffer
    (main.cpp:2165-2179) writes it to the frame's UBO.  cameraSpeed = 5 / FPS in the reference;
    `speed` fixes it per frame."""
    out = np.repeat(ubo[None], n, axis=0).copy()
    base = np.array(ubo["camPos"][:3], np.float32)
    for k in range(n):
        out[k]["camPos"][:3] = base + np.float32(speed) * np.array([k, 0.0, -k], np.float32)
    return out


# ---- views (abi.h trt_view) --------------------------------------------------------------

VIEW_IDENTITY = np.zeros((), T.VIEW)
VIEW_IDENTITY["right"], VIEW_IDENTITY["up"], VIEW_IDENTITY["back"] = (1, 0, 0), (0, 1, 0), (0, 0, 1)


def _f3(v) -> ctypes.Array:
    return (ctypes.c_float * 3)(*[float(np.float32(x)) for x in v])


def view_look(front, up=(0.0, 1.0, 0.0)) -> np.ndarray:
    """The view of a camera looking along `front` (trt_view_look): the reference's cameraFront
    (0, 0, -1) and cameraUp (0, 1, 0) (main.cpp:342-344) give the reference camera's bytes."""
    v = np.zeros((), T.VIEW)
    rc = lib().trt_view_look(v.ctypes.data, _f3(front), _f3(up))
    if rc != 0:
        raise TrtError(rc, f"trt_view_look(front={tuple(front)}, up={tuple(up)}): zero, parallel or non-finite input")
    return v


def view_ypr(yaw: float, pitch: float, roll: float = 0.0) -> np.ndarray:
    """The view M = Ry(yaw) Rx(pitch) Rz(roll), angles in degrees: computed in double, rounded
    to float32; its columns are right, up, back.  (0, 0, 0) is the reference camera's bytes."""
    y, p, r = (np.deg2rad(np.float64(a)) for a in (yaw, pitch, roll))
    ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]], np.float64)
    rx = np.array([[1, 0, 0], [0, np.cos(p), -np.sin(p)], [0, np.sin(p), np.cos(p)]], np.float64)
    rz = np.array([[np.cos(r), -np.sin(r), 0], [np.sin(r), np.cos(r), 0], [0, 0, 1]], np.float64)
    m = ((ry @ rx @ rz) + 0.0).astype(np.float32)  # + 0.0: no negative zeros
    v = np.zeros((), T.VIEW)
    v["right"], v["up"], v["back"] = m[:, 0], m[:, 1], m[:, 2]
    return v


def view_rays(params: T.Params, view=None) -> np.ndarray:
    """The (height, width) Ray records a host would bind as binding 1 for `view` at spp 1
    (trt_view_rays; None = the reference camera): the bit-exact host twin of the kernel's view
    arithmetic, for replay through rays_in (draw_frame, the CPU oracle)."""
    p = T.Params.from_buffer_copy(params)
    out = np.zeros((p.height, p.width), T.RAY)
    v = None if view is None else np.ascontiguousarray(view, T.VIEW)
    rc = lib().trt_view_rays(ctypes.byref(p), None if v is None else v.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise TrtError(rc, "trt_view_rays: bad image size")
    return out


def pinhole_qrays(params: T.Params, view=None, cam=(0.0, 0.0, 0.0)) -> np.ndarray:
    """view_rays plus an origin: the (height, width) T.QRAY records of the pinhole camera at `cam`
    under `view`, for Renderer.trace_rays — the rays a frame of that view and camPos traces."""
    r = view_rays(params, view)
    q = np.zeros(r.shape, T.QRAY)
    q["dir"] = r["dir"][..., :3]
    q["org"] = np.asarray(cam, np.float32)
    return q


def equirect_qrays(width: int, height: int, cam=(0.0, 0.0, 0.0)) -> np.ndarray:
    """A 360-degree panorama camera at `cam`: (height, width) T.QRAY records whose directions go
    through the centres of the texels of a width x height equirectangular image — the inverse of
    the shader's direction_to_uv (shader.comp:410-416: u = (atan(z, x) + pi) / 2 pi, v = acos(y) /
    pi), computed in float64 and rounded once to float32 (the kernel normalizes)."""
    u = (np.arange(width, dtype=np.float64) + 0.5) / width
    v = (np.arange(height, dtype=np.float64) + 0.5) / height
    theta = (u * 2.0 * np.pi - np.pi)[None, :]
    phi = (v * np.pi)[:, None]
    q = np.zeros((height, width), T.QRAY)
    q["dir"][..., 0] = np.sin(phi) * np.cos(theta)
    q["dir"][..., 1] = np.cos(phi) * np.ones_like(theta)
    q["dir"][..., 2] = np.sin(phi) * np.sin(theta)
    q["org"] = np.asarray(cam, np.float32)
    return q


def segments_between(a, b) -> np.ndarray:
    """"Can a see b": the T.QSEG records of Renderer.occluded for the segments from points `a` to
    points `b` ((..., 3) each, broadcast against each other): org = a, dir = b - a and tmax =
    |b - a|, all in float32 — the length as sqrt((x * x + y * y) + z * z) in the project's dot
    order, the sum the kernel normalizes the direction by.  A surface at b itself does not occlude
    (the test is t < tmax); start a little off a surface at a, as the shader's shadow rays do."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    a, b = np.broadcast_arrays(a, b)
    if a.shape[-1] != 3:
        raise ValueError("points are (..., 3) arrays")
    d = (b - a).astype(np.float32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    s = np.zeros(a.shape[:-1], T.QSEG)
    s["org"] = a
    s["dir"] = d
    s["tmax"] = np.sqrt((x * x + y * y) + z * z, dtype=np.float32)
    return s


def segments_from_rays(qrays, tmax=T.QSEG_MAX_T) -> np.ndarray:
    """T.QRAY records as T.QSEG records of the same shape: origin and direction copied, cut off at
    `tmax` (a scalar or one per ray; the default is a whole ray: occluded = the ray hits anything)."""
    r = np.asarray(qrays, T.QRAY)
    s = np.zeros(r.shape, T.QSEG)
    s["org"] = r["org"]
    s["dir"] = r["dir"]
    s["tmax"] = np.asarray(tmax, np.float32)
    return s


def sphere_dirs(k: int) -> np.ndarray:
    """`k` unit directions spread evenly over the sphere (a Fibonacci spiral about the y axis, from
    near +y to near -y), (k, 3) float32, computed in float64 and rounded once.  With
    Renderer.visibility(..., dirs=) each is turned into the hemisphere of a point's normal, so k
    directions sample that hemisphere k times (ambient occlusion = popcount(mask) / k)."""
    if k < 1:
        raise ValueError("at least one direction")
    i = np.arange(k, dtype=np.float64)
    y = 1.0 - (2.0 * i + 1.0) / k
    r = np.sqrt(1.0 - y * y)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))  # the golden angle
    d = np.stack([r * np.cos(phi), y, r * np.sin(phi)], 1)
    d /= np.sqrt((d * d).sum(1))[:, None]
    return d.astype(np.float32)


def points_on_hits(rays, hits, offset: float = 1e-3, tmax=T.QSEG_MAX_T) -> tuple[np.ndarray, np.ndarray]:
    """One T.QPOINT per ray that hit something (Renderer.trace_rays' T.QHIT records): the hit point
    org + t normalize(dir), moved `offset` along the record's normal turned against the ray, with
    that turned normal as the point's n — the place a shader's secondary rays start from.
    Computed in float64 and rounded once.  Returns (points, the ray index of each point)."""
    r = np.asarray(rays, T.QRAY).reshape(-1)
    h = np.asarray(hits, T.QHIT).reshape(-1)
    if len(r) != len(h):
        raise ValueError("one hit record per ray")
    idx = np.flatnonzero((h["kind"] != T.HIT_NONE) & (h["kind"] != T.HIT_BAD_RAY))
    o = r["org"][idx].astype(np.float64)
    d = r["dir"][idx].astype(np.float64)
    d /= np.sqrt((d * d).sum(1))[:, None]
    n = h["n"][idx].astype(np.float64)
    n = np.where(((n * d).sum(1) > 0.0)[:, None], -n, n)
    pts = np.zeros(len(idx), T.QPOINT)
    pts["pos"] = o + h["t"][idx].astype(np.float64)[:, None] * d + float(offset) * n
    pts["n"] = n
    pts["tmax"] = np.asarray(tmax, np.float32)
    return pts, idx


def visibility_set(dirs=None, targets=None) -> tuple[int, np.ndarray]:
    """(mode, the (K, 4) float32 set array of trt_visibility) from exactly one of `dirs` /
    `targets`, (K, 3) or (K, 4) arrays (a fourth column is carried and ignored)."""
    if (dirs is None) == (targets is None):
        raise ValueError("exactly one of dirs= and targets=")
    a = np.asarray(dirs if targets is None else targets, np.float32)
    if a.ndim != 2 or a.shape[1] not in (3, 4):
        raise ValueError("a direction or target set is a (K, 3) or (K, 4) array")
    e = np.zeros((a.shape[0], 4), np.float32)
    e[:, : a.shape[1]] = a
    return (T.VIS_DIRS if targets is None else T.VIS_TARGETS), e


def point_segments(points, dirs=None, targets=None) -> np.ndarray:
    """The (npoints, K) T.QSEG records Renderer.visibility traces for `points` (T.QPOINT) and a
    direction or target set, exactly as the kernel forms them (trt_point_segments):
    visibility bit k of point i == Renderer.occluded of record [i, k].  A target record that is
    not a valid segment (a point on its target) is returned as computed; its bit reads 0."""
    mode, e = visibility_set(dirs, targets)
    p = np.ascontiguousarray(points, T.QPOINT).reshape(-1)
    out = np.zeros((len(p), len(e)), T.QSEG)
    rc = lib().trt_point_segments(p.ctypes.data if len(p) else None, len(p), e.ctypes.data if len(e) else None, len(e),
                                  mode, out.ctypes.data if out.size else None)
    if rc != 0:
        raise TrtError(rc, "trt_point_segments: a point or set entry is not valid, or the set does not hold 1..63 entries")
    return out


def inside_length(hits, counts) -> np.ndarray:
    """The length each segment of a Renderer.trace_all answer spends inside closed meshes: its
    triangle records, in order, are paired (first with second, third with fourth, ...) and the
    differences of t summed, in float64; an unpaired last crossing adds nothing.  Floor and sphere
    records are left out.  Meaningful for origins outside the meshes (a segment that starts
    inside pairs its exit with the next entry) and for answers that are not truncated
    (crossing_parity).  `hits` is (n, K) T.QHIT, `counts` (n,); returns (n,) float64."""
    h = np.asarray(hits, T.QHIT)
    c = np.asarray(counts).astype(np.uint32).reshape(-1)
    if h.ndim != 2 or h.shape[0] != len(c):
        raise ValueError("hits are (n, K) T.QHIT records and counts (n,)")
    m = np.where(c == T.ALLHITS_BAD_SEG, 0, c & 0x7FFFFFFF)
    tri = (np.arange(h.shape[1])[None, :] < m[:, None]) & (h["kind"] == T.HIT_TRIANGLE)
    rank = np.cumsum(tri, 1) - 1  # the index of a triangle record among its segment's
    ntri = tri.sum(1)
    paired = tri & (rank < (ntri - ntri % 2)[:, None])
    sign = np.where(rank % 2 == 1, 1.0, -1.0)
    return np.where(paired, sign * h["t"].astype(np.float64), 0.0).sum(1)


def crossing_parity(counts) -> tuple[np.ndarray, np.ndarray]:
    """(odd, truncated) of a Renderer.trace_all count array: whether the number of crossings is
    odd (a point inside a closed mesh, for a whole ray from it), and whether the count carries
    T.ALLHITS_MORE, in which case the parity is that of max_hits and says nothing.  A bad record
    (T.ALLHITS_BAD_SEG) is reported as truncated."""
    c = np.asarray(counts).astype(np.uint32)
    return (c & 1).astype(bool) & (c != T.ALLHITS_BAD_SEG), (c & T.ALLHITS_MORE) != 0


def camera_orbit(ubo: np.ndarray, n: int, speed: float = 0.02, yaw_step: float = 1.0, pitch_step: float = -0.25,
                 yaw0: float = 0.0, pitch0: float = 0.0) -> tuple[np.ndarray, np.ndarray]:
    """camera_path with a camera that turns while it walks (mouse look held with W and D): n
    per-frame UBOs and n views, frame k looking along view_ypr(yaw0 + k * yaw_step, pitch0 + k *
    pitch_step).  For render_frames(..., ubos=, views=)."""
    views = np.zeros(n, T.VIEW)
    for k in range(n):
        views[k] = view_ypr(yaw0 + k * yaw_step, pitch0 + k * pitch_step, 0.0)
    return camera_path(ubo, n, speed), views


# ---- synthetic inputs --------------------------------------------------------------------


def _hash32(x: np.ndarray) -> np.ndarray:
    """PCG-style integer hash (uint32, vectorised)."""
    x = x.astype(np.uint32)
    state = x * np.uint32(747796405) + np.uint32(2891336453)
    word = ((state >> ((state >> np.uint32(28)) + np.uint32(4))) ^ state) * np.uint32(277803737)
    return (word >> np.uint32(22)) ^ word


def synthetic_envmap(width: int = 7616, height: int = 3808, seed: int = 0) -> np.ndarray:
    """Seeded procedural equirectangular RGBA8 envmap (H, W, 4), a stand-in with the shape of
    the reference's background.jpg (7616x3808, main.cpp:928-949): sky gradient over a darker
    ground, a longitude/latitude grid and per-texel hashed noise, so bilinear filtering sees
    texel-scale detail.  Deterministic for (width, height, seed)."""
    with np.errstate(over="ignore"):
        out = np.empty((height, width, 4), np.uint8)
        xs = np.arange(width, dtype=np.uint32)
        hx = _hash32(xs ^ np.uint32(seed * 0x9E3779B9 & 0xFFFFFFFF))
        grid_x = (xs % np.uint32(256)) < np.uint32(6)
        for y0 in range(0, height, 512):
            ys = np.arange(y0, min(height, y0 + 512), dtype=np.uint32)
            v = (ys.astype(np.float32) + 0.5) / np.float32(height)
            n = _hash32(hx[None, :] + ys[:, None] * np.uint32(0x85EBCA6B))
            noise = (n & np.uint32(31)).astype(np.int32) - 16
            sky = v[:, None] < 0.5
            t = np.abs(v - 0.5)[:, None] * 2.0
            r = np.where(sky, 120 + 100 * t, 90 - 40 * t)
            g = np.where(sky, 170 + 60 * t, 70 - 30 * t)
            b = np.where(sky, 230 - 20 * t, 50 - 20 * t)
            grid = grid_x[None, :] | ((ys % np.uint32(256)) < np.uint32(6))[:, None]
            r = np.where(grid, 250, r) + noise
            g = np.where(grid, 240, g) + ((noise * 3) >> 2)
            b = np.where(grid, 200, b) + (noise >> 1)
            sl = slice(y0, y0 + len(ys))
            out[sl, :, 0] = np.clip(r, 0, 255).astype(np.uint8)
            out[sl, :, 1] = np.clip(g, 0, 255).astype(np.uint8)
            out[sl, :, 2] = np.clip(b, 0, 255).astype(np.uint8)
            out[sl, :, 3] = 255
    return out


def icosphere(level: int) -> tuple[np.ndarray, np.ndarray]:
    """Unit icosphere: 20 * 4**level triangles (level 4 = 5,120).  Returns float32 (V,3)
    positions and uint32 (F,3) indices, deterministic."""
    t = (1.0 + 5.0**0.5) / 2.0
    verts = [
        (-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0),
        (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
        (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1),
    ]
    verts = [np.array(v, np.float64) / np.linalg.norm(v) for v in verts]
    faces = [
        (0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11),
        (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
        (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9),
        (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1),
    ]
    for _ in range(level):
        cache: dict = {}

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                cache[key] = len(verts) - 1
            return cache[key]

        nf = []
        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nf
    return np.asarray(verts, np.float32), np.asarray(faces, np.uint32)


# ---- scene assembly ---------------------------------------------------------------------


class SceneBuilder:
    """The reference's per-model loop of createShaderStorageBuffers() (main.cpp:1533-1567),
    run by the product's C++ builder (trt_scene_*)."""

    def __init__(self, batch_size: int = 64):
        self._L = lib()
        h = ctypes.c_void_p()
        rc = self._L.trt_scene_create(ctypes.byref(h))
        if rc != 0:
            raise TrtError(rc, "trt_scene_create failed")
        self._h = h
        if batch_size != 64:
            self._check(self._L.trt_scene_set_batch_size(self._h, batch_size))

    def _check(self, rc: int):
        if rc != 0:
            raise TrtError(rc, self._L.trt_scene_last_error(self._h).decode())

    @staticmethod
    def _f3(v) -> ctypes.Array:
        return (ctypes.c_float * 3)(*[float(np.float32(x)) for x in v])

    def add_mesh(self, positions, indices, mat, scale=(1, 1, 1), rotation=(0, 0, 0),
                 translation=(0, 0, 0), normal_interp: int = 1) -> "SceneBuilder":
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
        m = np.ascontiguousarray(np.asarray(mat, T.MATERIAL).reshape(()))
        self._check(self._L.trt_scene_add_mesh(
            self._h, pos.ctypes.data, pos.shape[0], idx.ctypes.data, idx.shape[0], m.ctypes.data,
            self._f3(scale), self._f3(rotation), self._f3(translation), int(normal_interp)))
        return self

    def add_obj(self, path, mat, scale=(1, 1, 1), rotation=(0, 0, 0), translation=(0, 0, 0),
                normal_interp: int = 1) -> "SceneBuilder":
        m = np.ascontiguousarray(np.asarray(mat, T.MATERIAL).reshape(()))
        self._check(self._L.trt_scene_add_obj(
            self._h, str(path).encode(), m.ctypes.data, self._f3(scale), self._f3(rotation),
            self._f3(translation), int(normal_interp)))
        return self

    def add_model(self, info: ModelInfo, positions, indices) -> "SceneBuilder":
        return self.add_mesh(positions, indices, info.material, info.scale, info.rotation,
                             info.translation, info.normal_interp)

    def arrays(self) -> tuple[np.ndarray, np.ndarray]:
        nt = self._L.trt_scene_triangle_count(self._h)
        nm = self._L.trt_scene_model_count(self._h)
        tris = np.zeros(nt, T.TRIANGLE)
        models = np.zeros(nm, T.MODEL)
        if nt:
            ctypes.memmove(tris.ctypes.data, self._L.trt_scene_triangles(self._h), nt * T.TRIANGLE.itemsize)
        if nm:
            ctypes.memmove(models.ctypes.data, self._L.trt_scene_models(self._h), nm * T.MODEL.itemsize)
        return tris, models

    def close(self):
        if self._h:
            self._L.trt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class Scene:
    """Everything the reference binds for one frame (bindings 0, 4, 5, 6) plus the render
    settings of a configuration."""

    name: str
    ubo: np.ndarray
    tris: np.ndarray = field(default_factory=lambda: np.zeros(0, T.TRIANGLE))
    models: np.ndarray = field(default_factory=lambda: np.zeros(0, T.MODEL))
    env: np.ndarray | None = None  # (H, W, 4) uint8
    width: int = 1024
    height: int = 768
    max_depth: int = 20
    spp: int = 1
    flags: int = T.FLAGS_REFERENCE

    def params(self, **kw) -> T.Params:
        args = dict(width=self.width, height=self.height, max_depth=self.max_depth, spp=self.spp,
                    flags=self.flags)
        args.update(kw)
        return T.make_params(**args)


GOLDEN_MESHES = Path(__file__).resolve().parent.parent / "tests" / "golden" / "meshes.npz"


def load_golden_meshes(path: Path = GOLDEN_MESHES) -> dict:
    """Positions + triangulated indices of the reference assets as parsed by the reference's
    own tinyobjloader (tests/golden/make_goldens.py)."""
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def build_models(names, meshes: dict, batch_size: int = 64) -> tuple[np.ndarray, np.ndarray]:
    b = SceneBuilder(batch_size)
    for n in names:
        info = MODEL_INFOS[n]
        key = info.asset
        b.add_model(info, meshes[f"{key}:pos"], meshes[f"{key}:idx"])
    out = b.arrays()
    b.close()
    return out


_ENV_CACHE: dict = {}


def cached_envmap(width: int, height: int, seed: int = 0) -> np.ndarray:
    k = (width, height, seed)
    if k not in _ENV_CACHE:
        _ENV_CACHE[k] = synthetic_envmap(width, height, seed)
    return _ENV_CACHE[k]


def config_c1(width=1024, height=768) -> Scene:
    """C1: 4 spheres + checker floor, depth 1, no meshes, constant background (the CPU
    tinyraytracer reference case)."""
    return Scene("C1", make_ubo(), width=width, height=height, max_depth=1,
                 flags=T.FLAG_SPHERES | T.FLAG_FLOOR | T.FLAG_CHECKER | T.FLAG_ROW_QUIRK)


def config_c2(width=1024, height=768, env_size=(7616, 3808), seed=0) -> Scene:
    """C2 (headline): 4 spheres + plain floor + seeded envmap at the reference texture size,
    depth 4."""
    return Scene("C2", make_ubo(), env=cached_envmap(*env_size, seed), width=width, height=height,
                 max_depth=4, flags=T.FLAG_SPHERES | T.FLAG_FLOOR | T.FLAG_ENVMAP | T.FLAG_ROW_QUIRK)


def config_c3(width=1920, height=1080, env_size=(7616, 3808), level=4) -> Scene:
    """C3: spheres + one icosphere mesh (level 4 = 5,120 tris, 80 batches) in the reference's
    glass mesh material, depth 4."""
    pos, idx = icosphere(level)
    b = SceneBuilder()
    b.add_mesh(pos, idx, GLASS_MESH_MAT, scale=(1.5, 1.5, 1.5), translation=(2.5, -2.0, -10.0), normal_interp=1)
    tris, models = b.arrays()
    b.close()
    return Scene("C3", make_ubo(), tris, models, cached_envmap(*env_size), width, height, 4,
                 flags=T.FLAG_SPHERES | T.FLAG_FLOOR | T.FLAG_ENVMAP | T.FLAG_ROW_QUIRK)


C4_MATERIALS = (GLASS_MESH_MAT, WHISKY_MAT, ICE_MAT, BUNNY_MAT, DRAGON_MAT, FUDANLOGO_MAT, VENUS_MAT, DUCK_MAT)


def config_c4(width=3840, height=2160, env_size=(7616, 3808), n_objects=20, level=4, spp=1) -> Scene:
    """C4: ~100k triangles (20 level-4 icospheres = 102,400 tris / 1,600 batches) on a 5x4
    grid with the config.hpp mesh materials, spheres, floor, envmap, depth 4."""
    pos, idx = icosphere(level)
    b = SceneBuilder()
    for k in range(n_objects):
        gx, gz = k % 5, k // 5
        tr = (-6.0 + 3.0 * gx, -3.0 + 0.5 * (k % 3), -7.0 - 4.0 * gz)
        b.add_mesh(pos, idx, C4_MATERIALS[k % len(C4_MATERIALS)], scale=(1.0, 1.0, 1.0), translation=tr,
                   normal_interp=1 if k % 2 == 0 else 0)
    tris, models = b.arrays()
    b.close()
    return Scene("C4" if spp == 1 else "C5", make_ubo(), tris, models, cached_envmap(*env_size), width, height,
                 4, spp=spp, flags=T.FLAG_SPHERES | T.FLAG_FLOOR | T.FLAG_ENVMAP | T.FLAG_ROW_QUIRK)


def config_c5(width=3840, height=2160, env_size=(7616, 3808)) -> Scene:
    """C5: C4 with 16 PCG-jittered samples per pixel (build extension)."""
    return config_c4(width, height, env_size, spp=16)


def config_reference_default(meshes: dict | None = None, env_size=(7616, 3808), width=1024, height=768) -> Scene:
    """The shipped reference frame: glass + water + ice (37,956 tris / 594 batches, config.hpp:97),
    floor on, spheres off (shader.comp:83-84), envmap background, MAX_DEPTH 20, host ray quirk."""
    meshes = meshes if meshes is not None else load_golden_meshes()
    tris, models = build_models(DEFAULT_MODEL_LIST, meshes)
    return Scene("reference", make_ubo(), tris, models, cached_envmap(*env_size), width, height, 20,
                 flags=T.FLAGS_REFERENCE)


def config_readme(meshes: dict | None = None, env_size=(7616, 3808), width=1024, height=768,
                  max_depth=20) -> Scene:
    """The README-era scene that carries the reference's only published frame rate (10-11 FPS
    on an RTX 4060 at 1024x768, README.md:334-340): asschercut + bunny + dragon + venus +
    fudanlogo (config.hpp:96; 53,877 tris / 844 batches, rotated and flat-shaded models),
    checker floor, spheres off, envmap background, MAX_DEPTH 20 (shader.comp:75).  The README
    screenshots come from an older shader state, so the published figure is context only."""
    meshes = meshes if meshes is not None else load_golden_meshes()
    tris, models = build_models(README_MODEL_LIST, meshes)
    return Scene("readme", make_ubo(), tris, models, cached_envmap(*env_size), width, height, max_depth,
                 flags=T.FLAG_FLOOR | T.FLAG_CHECKER | T.FLAG_ENVMAP | T.FLAG_ROW_QUIRK)


CONFIGS = {"C1": config_c1, "C2": config_c2, "C3": config_c3, "C4": config_c4, "C5": config_c5}
