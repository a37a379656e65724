"""Byte layouts of the reference's scene records (include/trt/scene_types.h) as numpy
dtypes, plus the ctypes views of the C-ABI parameter structs (include/trt/abi.h).

Reference records: Material/Sphere/Triangle/Model (geometry.hpp:5-46, shader.comp:3-38),
UniformBufferObject and Ray (main.cpp:145-187, shader.comp:14-17, 40-51).
"""
from __future__ import annotations

import ctypes

import numpy as np

F4 = ("<f4", (4,))

MATERIAL = np.dtype([("albedo", *F4), ("diffuse_specular", *F4), ("refractive", *F4)])
SPHERE = np.dtype([("center_radius", *F4), ("material", MATERIAL)])
TRIANGLE = np.dtype(
    [
        ("v0", *F4),
        ("v1", *F4),
        ("v2", *F4),
        ("material", MATERIAL),
        ("v0_norm", *F4),
        ("v1_norm", *F4),
        ("v2_norm", *F4),
    ]
)
MODEL = np.dtype(
    [("params0", "<i4", (4,)), ("bboxMin", *F4), ("bboxMax", *F4), ("material", MATERIAL)]
)
UBO = np.dtype(
    [
        ("sphere0", SPHERE),
        ("sphere1", SPHERE),
        ("sphere2", SPHERE),
        ("sphere3", SPHERE),
        ("light0", *F4),
        ("light1", *F4),
        ("light2", *F4),
        ("camPos", *F4),
        ("bboxMin", *F4),
        ("bboxMax", *F4),
    ]
)
RAY = np.dtype([("dir", *F4), ("resultColor", *F4)])
# trt_view (abi.h): the columns of the camera-to-world rotation, back = -front
VIEW = np.dtype([("right", "<f4", (3,)), ("up", "<f4", (3,)), ("back", "<f4", (3,))])
MAX_VIEW_FRAMES = 32  # TRT_MAX_VIEW_FRAMES: frames of a launch with an oriented frame

# trt_qray / trt_qhit (abi.h): one ray of a query (Renderer.trace_rays) and its nearest hit
QRAY = np.dtype([("org", "<f4", (3,)), ("pad0", "<f4"), ("dir", "<f4", (3,)), ("pad1", "<f4")])
QHIT = np.dtype([("t", "<f4"), ("kind", "<u4"), ("index", "<u4"), ("u", "<f4"), ("v", "<f4"), ("n", "<f4", (3,))])
HIT_NONE = 0  # t = 1e10, the rest 0
HIT_FLOOR = 1
HIT_SPHERE = 2  # index 0..3
HIT_TRIANGLE = 3  # index into the scene's triangle array; u, v weigh v1, v2
HIT_BAD_RAY = 0xFFFFFFFF  # a device-pointer query's record of a ray that is not valid
QRAY_MIN_LEN2 = np.float32(1e-30)  # TRT_QRAY_MIN_LEN2 / MAX_LEN2: bounds of the direction's squared length
QRAY_MAX_LEN2 = np.float32(1e30)
QRAY_MAX_RAYS = 1 << 28
# abi.h trt_qseg: a segment of an occlusion query (Renderer.occluded), a ray cut off at tmax
QSEG = np.dtype([("org", "<f4", (3,)), ("tmax", "<f4"), ("dir", "<f4", (3,)), ("pad", "<f4")])
OCC_VISIBLE = 0
OCC_OCCLUDED = 1
OCC_BAD_SEG = 0xFF  # a device-pointer query's byte for a segment that is not valid
QSEG_MAX_T = np.float32(1e10)  # TRT_QSEG_MAX_T: the shader's initial nearest distance, "a whole ray"
assert QSEG.itemsize == 32
# abi.h trt_trace_all: every crossing of a segment, in order (Renderer.trace_all)
ALLHITS_MAX = 32  # max_hits in 1..32
ALLHITS_MORE = 0x80000000  # in counts[i]: further hits exist inside tmax
ALLHITS_BAD_SEG = 0xFFFFFFFF  # a device-pointer query's count for a segment that is not valid
# abi.h trt_qpoint: a point of a visibility query (Renderer.visibility); n only chooses the side
# of a TRT_VIS_DIRS direction, tmax cuts a direction off and caps the range to a target
QPOINT = np.dtype([("pos", "<f4", (3,)), ("tmax", "<f4"), ("n", "<f4", (3,)), ("pad", "<f4")])
VIS_DIRS = 0  # set entries are directions, turned into the hemisphere of n
VIS_TARGETS = 1  # set entries are points (lights): segments from each point to each target
VIS_MAX_SET = 63
VIS_BAD_POINT = 0xFFFFFFFFFFFFFFFF  # a device-pointer query's mask of a point that is not valid (-1 as int64)
assert QPOINT.itemsize == 32

assert VIEW.itemsize == 36 and QRAY.itemsize == 32 and QHIT.itemsize == 32
assert MATERIAL.itemsize == 48 and SPHERE.itemsize == 64
assert TRIANGLE.itemsize == 144 and MODEL.itemsize == 96
assert UBO.itemsize == 352 and RAY.itemsize == 32

# trt_params.flags (abi.h)
FLAG_SPHERES = 1 << 0
FLAG_FLOOR = 1 << 1
FLAG_CHECKER = 1 << 2
FLAG_ENVMAP = 1 << 3
FLAG_ROW_QUIRK = 1 << 4
FLAG_DEVICE_PTRS = 1 << 5
FLAG_COUNT = 1 << 6
FLAG_TIMING = 1 << 7
FLAG_BATCH_WALK = 1 << 8
FLAG_SRGB_OUT = 1 << 9
FLAG_BAND_IN_PLACE = 1 << 10  # band rows written at their frame rows (device outputs)
FLAGS_REFERENCE = FLAG_FLOOR | FLAG_ENVMAP | FLAG_ROW_QUIRK

MAX_DEPTH_LIMIT = 20

# status codes
TRT_OK = 0
TRT_ERR_INVALID = -1
TRT_ERR_HIP = -2
TRT_ERR_NOSCENE = -3
TRT_ERR_OOM = -4
TRT_ERR_IO = -5


class Params(ctypes.Structure):
    """trt_params (abi.h)."""

    _fields_ = [
        ("width", ctypes.c_uint32),
        ("height", ctypes.c_uint32),
        ("max_depth", ctypes.c_uint32),
        ("spp", ctypes.c_uint32),
        ("seed", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("fov", ctypes.c_float),
        ("band_rows", ctypes.c_uint32),
        ("band_count", ctypes.c_uint32),
        ("band_index", ctypes.c_uint32),
        ("rays_in", ctypes.c_void_p),
    ]


class Stats(ctypes.Structure):
    """trt_stats (abi.h)."""

    _fields_ = [
        ("primary_rays", ctypes.c_uint64),
        ("secondary_rays", ctypes.c_uint64),
        ("shadow_rays", ctypes.c_uint64),
        ("misses", ctypes.c_uint64),
        ("tri_nearest", ctypes.c_uint64),
        ("sphere_tests", ctypes.c_uint64),
        ("batch_tests", ctypes.c_uint64),
        ("batch_hits", ctypes.c_uint64),
        ("tri_tests", ctypes.c_uint64),
        ("node_tests", ctypes.c_uint64),
        ("kernel_ms", ctypes.c_double),
        ("tri_past_a", ctypes.c_uint64),
        ("tri_past_u", ctypes.c_uint64),
        ("tri_past_v", ctypes.c_uint64),
        ("shadow_skipped", ctypes.c_uint64),
        ("skipped_sphere_tests", ctypes.c_uint64),
        ("skipped_box_tests", ctypes.c_uint64),
        ("skipped_tri_tests", ctypes.c_uint64),
        ("skipped_tri_past_a", ctypes.c_uint64),
        ("skipped_tri_past_u", ctypes.c_uint64),
        ("skipped_tri_past_v", ctypes.c_uint64),
    ]

    COUNTERS = ("primary_rays", "secondary_rays", "shadow_rays", "misses", "tri_nearest",
                "sphere_tests", "batch_tests", "batch_hits", "tri_tests", "node_tests",
                "tri_past_a", "tri_past_u", "tri_past_v", "shadow_skipped", "skipped_sphere_tests",
                "skipped_box_tests", "skipped_tri_tests", "skipped_tri_past_a", "skipped_tri_past_u",
                "skipped_tri_past_v")
    # counters that must equal the oracle's (the reference's work); batch_tests / node_tests
    # depend on the traversal (the kernel culls with a conservative hierarchy)
    EXACT = ("primary_rays", "secondary_rays", "shadow_rays", "misses", "tri_nearest",
             "sphere_tests")
    # with TRT_FLAG_BATCH_WALK the kernel also tests exactly the reference's batches/triangles
    EXACT_WALK = EXACT + ("batch_hits", "tri_tests")

    def as_dict(self) -> dict:
        d = {k: int(getattr(self, k)) for k in self.COUNTERS}
        d["kernel_ms"] = float(self.kernel_ms)
        return d


class BandLayout(ctypes.Structure):
    """trt_band_layout (abi.h): buffer shapes of a tiled batch."""

    _fields_ = [
        ("groups", ctypes.c_uint32),
        ("max_rows", ctypes.c_uint32),
        ("block_bytes", ctypes.c_uint64),
        ("local_bytes", ctypes.c_uint64),
        ("gather_bytes", ctypes.c_uint64),
    ]


class BandXfer(ctypes.Structure):
    """trt_band_xfer (abi.h): the compact band blocks one rank sends to one root."""

    _fields_ = [
        ("src", ctypes.c_uint32),
        ("dst", ctypes.c_uint32),
        ("frames", ctypes.c_uint32),
        ("groups", ctypes.c_uint32),
        ("first_slot", ctypes.c_uint32),
        ("pad", ctypes.c_uint32),
        ("src_offset", ctypes.c_uint64),
        ("dst_offset", ctypes.c_uint64),
        ("bytes", ctypes.c_uint64),
    ]


PLAN_SELF_GATHER = 1  # TRT_PLAN_SELF_GATHER
ROOT_ROTATE = -1  # TRT_ROOT_ROTATE

assert ctypes.sizeof(Params) == 48 and ctypes.sizeof(Stats) == 168
assert ctypes.sizeof(BandLayout) == 32 and ctypes.sizeof(BandXfer) == 48


def make_params(
    width: int = 1024,
    height: int = 768,
    max_depth: int = 20,
    spp: int = 1,
    seed: int = 0,
    flags: int = FLAGS_REFERENCE,
    fov: float = 1.05,
    band_rows: int = 0,
    band_count: int = 0,
    band_index: int = 0,
    rays_in: int | None = None,
) -> Params:
    """Defaults are the reference's (main.cpp:35-36, 1498; shader.comp:75)."""
    p = Params()
    p.width, p.height, p.max_depth, p.spp, p.seed = width, height, max_depth, spp, seed
    p.flags, p.fov = flags, fov
    p.band_rows, p.band_count, p.band_index = band_rows, band_count, band_index
    p.rays_in = rays_in
    return p


def output_rows(height: int, band_rows: int = 0, band_count: int = 0, band_index: int = 0) -> list[int]:
    """Image rows a banded render writes, in output order (trt_output_rows)."""
    if band_rows == 0 or band_count <= 1:
        return list(range(height))
    return [r for r in range(height) if (r // band_rows) % band_count == band_index]


def ptr(a: np.ndarray | None) -> ctypes.c_void_p | None:
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"], "arrays handed to the C-ABI must be C-contiguous"
    return ctypes.c_void_p(a.ctypes.data)
