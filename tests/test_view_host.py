"""The host side of the view basis (abi.h trt_view): trt_view_rays is the bit-exact host twin of
the kernel's view arithmetic, trt_view_look builds a basis from the reference's cameraFront /
cameraUp, and the identity replay closes the chain to the CPU oracle.  No GPU."""
from __future__ import annotations

import ctypes
import math
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as orc
from vkcomputeshader_tinyraytracer_amd import ABI_SYMBOLS, lib, scene as S, types as T

f32 = np.float32

V1 = S.view_ypr(20, -10, 5)
V2 = S.view_ypr(-35, -20, 0)
V3 = S.view_ypr(180, 0, 0)
SKEW = np.zeros((), T.VIEW)  # finite, neither unit nor orthogonal
SKEW["right"], SKEW["up"], SKEW["back"] = (1.2, 0.1, 0.0), (0.3, 0.9, -0.2), (0.1, -0.2, 1.5)
VIEWS = {"identity": S.VIEW_IDENTITY, "V1": V1, "V2": V2, "V3": V3, "SKEW": SKEW}


def np_view_rays(p: T.Params, view) -> np.ndarray:
    """Steps 1 and 2 of the view's arithmetic contract (abi.h) in numpy float32: every product
    and every sum is one float32 operation."""
    w, h = p.width, p.height
    dz = f32(-1.0 * (h / (2.0 * math.tan(float(p.fov) / 2.0))))  # main.cpp:1503, in double
    x = np.arange(w, dtype=f32)[None, :].repeat(h, 0)
    row = np.arange(h, dtype=f32)[:, None].repeat(w, 1)
    if p.flags & T.FLAG_ROW_QUIRK:
        row[:, w - 1] += f32(1)  # main.cpp:1501-1502: the last column takes the next row's dy
    dx = (x + f32(0.5)) - f32(w) * f32(0.5)
    dy = -(row + f32(0.5)) + f32(h) * f32(0.5)
    inv = f32(1) / np.sqrt((dx * dx + dy * dy) + dz * dz)
    c = [dx * inv, dy * inv, np.full_like(dx, dz) * inv]
    out = np.zeros((h, w), T.RAY)
    r, u, b = (np.asarray(view[k], f32) for k in ("right", "up", "back"))
    for a in range(3):
        out["dir"][..., a] = (c[0] * r[a] + c[1] * u[a]) + c[2] * b[a]
    out["dir"][..., 3] = 1
    return out


def test_abi_table_lists_the_view_symbols():
    for name in ("trt_view_look", "trt_view_rays", "trt_set_view", "trt_render_frames_view", "trt_multi_set_view"):
        assert name in ABI_SYMBOLS
        assert hasattr(lib(), name)
    from vkcomputeshader_tinyraytracer_amd._lib import ABI_VERSION

    header = (Path(__file__).resolve().parents[1] / "include" / "trt" / "abi.h").read_text()
    assert ABI_VERSION == 5 and f"#define TRT_ABI_VERSION {ABI_VERSION}\n" in header
    assert f"abi {ABI_VERSION})".encode() in lib().trt_version()


def test_view_ypr_zero_is_the_reference_camera():
    assert S.view_ypr(0, 0, 0).tobytes() == S.VIEW_IDENTITY.tobytes()
    for v in (V1, V2, V3):
        m = np.stack([v["right"], v["up"], v["back"]], 1).astype(np.float64)
        assert np.abs(m.T @ m - np.eye(3)).max() < 1e-6 and np.linalg.det(m) > 0.999


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("size", [(96, 64), (33, 17)])
@pytest.mark.parametrize("name", list(VIEWS))
def test_view_rays_bit_exact(name, size, quirk):
    flags = T.FLAG_FLOOR | (T.FLAG_ROW_QUIRK if quirk else 0)
    p = T.make_params(width=size[0], height=size[1], max_depth=4, spp=1, flags=flags)
    got = S.view_rays(p, VIEWS[name])
    want = np_view_rays(p, VIEWS[name])
    assert got.tobytes() == want.tobytes()
    if name == "identity":
        assert S.view_rays(p, None).tobytes() == want.tobytes()
    else:
        assert (got["dir"][..., :3] != S.view_rays(p, None)["dir"][..., :3]).any(-1).mean() > 0.5


@pytest.mark.parametrize("config", ["C1", "C2"])
def test_oracle_replays_identity_rays_bit_for_bit(config):
    sc = S.config_c1(96, 64) if config == "C1" else S.config_c2(96, 64, env_size=(64, 32))
    p = sc.params()
    want8, want32, wst = orc.render(sc, p, want32=True)
    rays = S.view_rays(p, S.VIEW_IDENTITY)
    q = sc.params()
    q.rays_in = rays.ctypes.data
    got8, got32, gst = orc.render(sc, q, want32=True)
    assert np.array_equal(got8, want8) and np.array_equal(got32, want32)
    wst.pop("kernel_ms", None), gst.pop("kernel_ms", None)
    assert gst == wst


def _look(front, up):
    v = np.zeros((), T.VIEW)
    fa = (ctypes.c_float * 3)(*front) if front is not None else None
    ua = (ctypes.c_float * 3)(*up) if up is not None else None
    return lib().trt_view_look(v.ctypes.data, fa, ua), v


def test_view_look():
    rc, v = _look((0, 0, -1), (0, 1, 0))  # cameraFront, cameraUp (main.cpp:342-344)
    assert rc == 0 and v.tobytes() == S.VIEW_IDENTITY.tobytes()
    assert S.view_look((0, 0, -1)).tobytes() == S.VIEW_IDENTITY.tobytes()
    for front in ((1.0, 0.0, -1.0), (-0.3, -0.5, -2.0), (0.2, 0.9, 0.4)):
        v = S.view_look(front)
        m = np.stack([v["right"], v["up"], v["back"]], 1).astype(np.float64)
        assert np.abs(m.T @ m - np.eye(3)).max() < 1e-6
        f = np.asarray(front, np.float64)
        assert np.abs(v["back"] + f / np.linalg.norm(f)).max() < 1e-6
        assert np.linalg.det(m) > 0  # right-handed: right x up = back
    nan = float("nan")
    for front, up in (((0, 0, 0), (0, 1, 0)), ((0, 0, -1), (0, 0, 0)), ((0, 2, 0), (0, 1, 0)), ((0, -1, 0), (0, 3, 0)),
                      ((nan, 0, -1), (0, 1, 0)), ((0, 0, -1), (0, float("inf"), 0)), (None, (0, 1, 0)),
                      ((0, 0, -1), None)):
        assert _look(front, up)[0] == T.TRT_ERR_INVALID, (front, up)
    assert lib().trt_view_look(None, (ctypes.c_float * 3)(0, 0, -1), (ctypes.c_float * 3)(0, 1, 0)) == T.TRT_ERR_INVALID


def test_view_rays_rejects_bad_arguments():
    p = T.make_params(width=8, height=8, max_depth=1, spp=1, flags=0)
    assert lib().trt_view_rays(ctypes.byref(p), None, None) == T.TRT_ERR_INVALID
    assert lib().trt_view_rays(None, None, None) == T.TRT_ERR_INVALID


def test_camera_orbit_turns_while_it_walks():
    ubo = S.make_ubo()
    ubos, views = S.camera_orbit(ubo, 5, speed=0.5, yaw_step=3.0, pitch_step=-1.0)
    assert ubos.shape == (5,) and views.shape == (5,) and views.dtype == T.VIEW
    assert np.array_equal(ubos, S.camera_path(ubo, 5, 0.5))
    assert views[0].tobytes() == S.VIEW_IDENTITY.tobytes()
    assert views[3].tobytes() == S.view_ypr(9.0, -3.0, 0.0).tobytes()
