"""The host side of the ray queries (abi.h trt_trace_rays): the ABI additions, trt_pixel_ray as the
single-pixel twin of trt_view_rays, the shared ray predicate behind trt_check_rays, the panorama
camera, and the register / scratch budget of the query kernels.  No GPU."""
from __future__ import annotations

import ctypes
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as orc
from vkcomputeshader_tinyraytracer_amd import ABI_SYMBOLS, lib, scene as S, types as T

f32 = np.float32
REPO = Path(__file__).resolve().parents[1]
OBJ = REPO / "build" / "csrc" / "trt_kernel.o"

SKEW = np.zeros((), T.VIEW)  # finite, neither unit nor orthogonal (the basis of test_view_host.py)
SKEW["right"], SKEW["up"], SKEW["back"] = (1.2, 0.1, 0.0), (0.3, 0.9, -0.2), (0.1, -0.2, 1.5)
VIEWS = {"identity": S.VIEW_IDENTITY, "V1": S.view_ypr(20, -10, 5), "SKEW": SKEW}


def test_abi_lists_the_query_symbols_and_keeps_its_version():
    for name in ("trt_trace_rays", "trt_check_rays", "trt_pixel_ray"):
        assert name in ABI_SYMBOLS
        assert hasattr(lib(), name)
    from vkcomputeshader_tinyraytracer_amd._lib import ABI_VERSION

    header = (REPO / "include" / "trt" / "abi.h").read_text()
    assert ABI_VERSION == 5 and "#define TRT_ABI_VERSION 5\n" in header
    assert T.QRAY.itemsize == 32 and T.QHIT.itemsize == 32
    assert {n: T.QRAY.fields[n][1] for n in T.QRAY.names} == {"org": 0, "pad0": 12, "dir": 16, "pad1": 28}
    assert {n: T.QHIT.fields[n][1] for n in T.QHIT.names} == {"t": 0, "kind": 4, "index": 8, "u": 12, "v": 16, "n": 20}
    # the header's constants, as the package mirrors them
    for name, val in (("TRT_HIT_NONE", T.HIT_NONE), ("TRT_HIT_FLOOR", T.HIT_FLOOR), ("TRT_HIT_SPHERE", T.HIT_SPHERE),
                      ("TRT_HIT_TRIANGLE", T.HIT_TRIANGLE)):
        assert re.search(rf"#define {name} {val}u\b", header), name
    assert "#define TRT_HIT_BAD_RAY 0xffffffffu" in header and T.HIT_BAD_RAY == 0xFFFFFFFF
    assert "#define TRT_QRAY_MIN_LEN2 1e-30f" in header and "#define TRT_QRAY_MAX_LEN2 1e30f" in header


def _pixel_ray(p, view, cam, x, y):
    out = np.zeros(1, T.QRAY)
    v = None if view is None else np.ascontiguousarray(view, T.VIEW)
    rc = lib().trt_pixel_ray(ctypes.byref(p), None if v is None else v.ctypes.data, (ctypes.c_float * 3)(*cam), x, y,
                             out.ctypes.data)
    return rc, out[0]


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("size", [(96, 64), (33, 17)])
@pytest.mark.parametrize("name", list(VIEWS))
def test_pixel_ray_is_the_twin_of_view_rays(name, size, quirk):
    w, h = size
    p = T.make_params(width=w, height=h, max_depth=4, spp=1, flags=T.FLAG_FLOOR | (T.FLAG_ROW_QUIRK if quirk else 0))
    rays = S.view_rays(p, VIEWS[name])
    cam = (f32(1.25), f32(-0.5), f32(3.0))
    pixels = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w - 1, h // 2), (w // 2, h // 3)]
    for x, y in pixels:
        rc, q = _pixel_ray(p, VIEWS[name], cam, x, y)
        assert rc == 0
        assert q["dir"].tobytes() == rays["dir"][y, x, :3].tobytes(), (x, y)
        assert q["org"].tobytes() == np.asarray(cam, f32).tobytes() and q["pad0"] == 0 and q["pad1"] == 0
    if name == "identity":  # a NULL view is the reference camera
        rc, q = _pixel_ray(p, None, cam, w - 1, 1)
        assert rc == 0 and q["dir"].tobytes() == rays["dir"][1, w - 1, :3].tobytes()
    full = S.pinhole_qrays(p, VIEWS[name], cam)
    assert full.shape == (h, w) and full["dir"].tobytes() == rays["dir"][..., :3].tobytes()
    assert (full["org"] == np.asarray(cam, f32)).all()
    assert _pixel_ray(p, VIEWS[name], cam, w, 0)[0] == T.TRT_ERR_INVALID
    assert _pixel_ray(p, VIEWS[name], cam, 0, h)[0] == T.TRT_ERR_INVALID
    assert lib().trt_pixel_ray(ctypes.byref(p), None, None, 0, 0, np.zeros(1, T.QRAY).ctypes.data) == T.TRT_ERR_INVALID


def _check(rays):
    r = np.ascontiguousarray(rays, T.QRAY).reshape(-1)
    bad = ctypes.c_uint32(0xDEAD)
    rc = lib().trt_check_rays(r.ctypes.data if len(r) else None, len(r), ctypes.byref(bad))
    return rc, bad.value


def _ray(org=(0.5, 1.0, -2.0), d=(0.0, 0.0, -1.0)):
    q = np.zeros(1, T.QRAY)
    q["org"], q["dir"] = org, d
    return q


def np_valid(r: np.ndarray) -> np.ndarray:
    """The predicate of trt_qray.h in float32 numpy: six finite floats and the direction's squared
    length, summed in the project's dot order, within [QRAY_MIN_LEN2, QRAY_MAX_LEN2]."""
    with np.errstate(all="ignore"):
        d = r["dir"].astype(f32)
        s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return (np.isfinite(r["org"]).all(-1) & np.isfinite(d).all(-1) & (s >= T.QRAY_MIN_LEN2) & (s <= T.QRAY_MAX_LEN2))


def test_check_rays():
    assert _check(np.zeros(0, T.QRAY)) == (0, 0)
    assert lib().trt_check_rays(None, 3, None) == T.TRT_ERR_INVALID
    for length in (1.0, 1e-3, 1e3):  # the kernel normalizes: any ordinary length is accepted
        assert _check(_ray(d=(0.6 * length, 0.0, -0.8 * length)))[0] == 0, length
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(6):
            q = _ray(d=(0.1, 0.2, -1.0))
            (q["org"] if k < 3 else q["dir"])[0, k % 3] = bad
            assert _check(q)[0] == T.TRT_ERR_INVALID, (bad, k)
    assert _check(_ray(d=(0.0, 0.0, 0.0)))[0] == T.TRT_ERR_INVALID
    assert _check(_ray(d=(0.0, 1e-16, 0.0)))[0] == T.TRT_ERR_INVALID  # s = 1e-32 < the minimum
    assert _check(_ray(d=(0.0, 0.0, 1e16)))[0] == T.TRT_ERR_INVALID   # s = 1e32 > the maximum
    assert _check(_ray(d=(3e19, 0.0, 0.0)))[0] == T.TRT_ERR_INVALID   # s overflows to inf
    # the lowest bad index
    many = np.concatenate([_ray()] * 9)
    many["dir"][7] = 0
    many["org"][4, 1] = np.nan
    assert _check(many) == (T.TRT_ERR_INVALID, 4)
    many["org"][4, 1] = 0
    assert _check(many) == (T.TRT_ERR_INVALID, 7)


def test_check_rays_agrees_with_the_numpy_predicate_on_random_bits():
    rng = np.random.default_rng(20260)
    n = 10000
    r = np.zeros(n, T.QRAY)
    bits = rng.integers(0, 2**32, size=(n, 6), dtype=np.uint64).astype(np.uint32)
    # half the rays keep an ordinary exponent in most fields, so both verdicts are well populated
    tame = rng.random((n, 6)) < 0.45
    bits = np.where(tame, (bits & np.uint32(0x807FFFFF)) | (rng.integers(90, 165, size=(n, 6)).astype(np.uint32) << 23), bits)
    fl = bits.view(f32)
    r["org"], r["dir"] = fl[:, :3], fl[:, 3:]
    want = np_valid(r)
    assert 0.1 < want.mean() < 0.9
    L = lib()
    got = np.array([L.trt_check_rays(r[i:i + 1].ctypes.data, 1, None) == 0 for i in range(n)])
    assert np.array_equal(got, want)
    assert _check(r) == (T.TRT_ERR_INVALID, int(np.argmin(want)))
    assert _check(r[want]) == (0, 0)


def test_equirect_qrays():
    w, h, cam = 64, 32, (1.0, 2.0, -3.0)
    q = S.equirect_qrays(w, h, cam)
    assert q.shape == (h, w) and q.dtype == T.QRAY
    assert np.isfinite(q["dir"]).all() and (q["org"] == np.asarray(cam, f32)).all()
    assert _check(q) == (0, 0)
    for y in range(h):
        for x in range(w):
            u, v = orc.direction_to_uv(q["dir"][y, x])
            assert abs(u * w - (x + 0.5)) < 0.5 and abs(v * h - (y + 0.5)) < 0.5, (x, y, u, v)


@pytest.fixture(scope="module")
def resources():
    # a missing object is a failed or skipped kernel build, not a missing GPU: fail, do not skip
    assert OBJ.exists(), "build/csrc/trt_kernel.o is missing: run __graft_entry__.build() first"
    out = subprocess.run([sys.executable, str(REPO / "tools" / "kres.py"), "ray_query_kernel"], check=True,
                         capture_output=True, text=True).stdout
    res = {}
    for line in out.splitlines():
        m = re.match(r"void trt::ray_query_kernel<([^>]*)>\(trt::KArgs.*\)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+lds\s+(\d+)",
                     line)
        if m:
            res[m.group(1)] = dict(vgpr=int(m.group(2)), sgpr=int(m.group(3)), scratch=int(m.group(4)),
                                   lds=int(m.group(5)))
    assert res, out[:500]
    return res


def test_query_kernel_resources(resources):
    """<CAP, COUNT, GEOM, SHADE>: the depth-4 triangle-free query kernel keeps the 5-wave budget of
    the C2 frame kernel (96 VGPRs, no scratch); the depth-4 quantized-BVH one stays at the scratch
    this build measured, 384 B (its frame twin: 432 B, test_c4_kernel_scratch_budget)."""
    r = resources["3, false, 0, true"]
    assert r["vgpr"] <= 96 and r["scratch"] == 0, r
    r = resources["3, false, 3, true"]
    assert r["vgpr"] <= 96 and r["scratch"] <= 384, r
    # every geometry path has its hits-only kernel, and none of them shades (no segment stack in LDS)
    for g in range(4):
        assert f"0, false, {g}, false" in resources
    assert resources["0, false, 0, false"]["lds"] == 0
