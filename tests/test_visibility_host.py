"""The host side of the visibility masks (abi.h trt_visibility): the ABI additions, the shared point
predicate behind trt_check_points, trt_point_segments — the host twin of the segments the kernel
forms — against a float32 numpy restatement, and the helpers of the scene module.  No GPU."""
from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.query_common import random_rays
from vkcomputeshader_tinyraytracer_amd import ABI_SYMBOLS, LIB_PATH, TrtError, lib, scene as S, types as T

f32 = np.float32
REPO = Path(__file__).resolve().parents[1]
HEADER = (REPO / "include" / "trt" / "abi.h").read_text()
TINY = np.nextafter(f32(0), f32(1))  # the smallest positive subnormal


def test_sizes_and_constants():
    m = re.search(r"typedef struct trt_qpoint \{([^}]*)\} trt_qpoint;", HEADER)
    assert m, "trt_qpoint is not declared"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "float pos[3]; float tmax; float n[3]; float pad;"
    assert "static_assert(sizeof(trt_qpoint) == 32" in HEADER
    assert T.QPOINT.itemsize == 32
    assert {n: T.QPOINT.fields[n][1] for n in T.QPOINT.names} == {"pos": 0, "tmax": 12, "n": 16, "pad": 28}
    assert all(T.QPOINT.fields[n][0].base == np.dtype("<f4") for n in T.QPOINT.names)
    for name, val in (("TRT_VIS_DIRS", "0u"), ("TRT_VIS_TARGETS", "1u"), ("TRT_VIS_MAX_SET", "63u"),
                      ("TRT_VIS_BAD_POINT", "0xffffffffffffffffull")):
        assert re.search(rf"#define {name} +{val}(\s|$)", HEADER, flags=re.M), name
    assert (T.VIS_DIRS, T.VIS_TARGETS, T.VIS_MAX_SET, T.VIS_BAD_POINT) == (0, 1, 63, 2**64 - 1)
    assert np.uint64(T.VIS_BAD_POINT).astype(np.int64) == -1  # what a torch.int64 tensor shows


def test_exports_and_version():
    from vkcomputeshader_tinyraytracer_amd._lib import ABI_VERSION

    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (trt_\w+)", out))
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("trt_visibility", "trt_check_points", "trt_point_segments"):
        assert name in exported and name in ABI_SYMBOLS and hasattr(lib(), name)
        assert re.search(rf"\bint {name}\s*\(", code), name
    assert ABI_VERSION == 5 and "#define TRT_ABI_VERSION 5\n" in HEADER
    assert b"visibility_query_kernel" in LIB_PATH.read_bytes()  # the kernel is in the code object


# ---- trt_check_points -------------------------------------------------------------------------------


def _check(pts):
    p = np.ascontiguousarray(pts, T.QPOINT).reshape(-1)
    bad = ctypes.c_uint32(0xDEAD)
    rc = lib().trt_check_points(p.ctypes.data if len(p) else None, len(p), ctypes.byref(bad))
    return rc, bad.value


def _pt(pos=(0.5, 1.0, -2.0), n=(0.0, 1.0, 0.0), tmax=3.0):
    q = np.zeros(1, T.QPOINT)
    q["pos"], q["n"], q["tmax"] = pos, n, tmax
    return q


def test_check_points_valid_edges():
    assert _check(np.zeros(0, T.QPOINT)) == (0, 0)
    assert TINY > 0 and TINY == f32(1.4e-45)
    for tmax in (TINY, f32(1e-4), f32(1.0), f32(1e10)):
        assert _check(_pt(tmax=tmax)) == (0, 0), tmax
    # n only chooses a side: zero, tiny and huge normals are all valid
    for n in ((0.0, 0.0, 0.0), (-0.0, 0.0, 0.0), (1e-30, 0.0, 0.0), (0.0, 3e38, 0.0)):
        assert _check(_pt(n=n)) == (0, 0), n


def test_check_points_invalid_edges():
    assert lib().trt_check_points(None, 3, None) == T.TRT_ERR_INVALID
    bad = ctypes.c_uint32(0xDEAD)
    assert lib().trt_check_points(None, 3, ctypes.byref(bad)) == T.TRT_ERR_INVALID and bad.value == 0
    over = np.nextafter(f32(1e10), f32(np.inf))
    assert over > f32(1e10)
    for tmax in (f32(0.0), f32(-0.0), f32(-1.0), over, f32(np.inf), f32(-np.inf), f32(np.nan)):
        assert _check(_pt(tmax=tmax)) == (T.TRT_ERR_INVALID, 0), tmax
    for v in (float("nan"), float("inf"), -float("inf")):
        for k in range(6):
            q = _pt()
            (q["pos"] if k < 3 else q["n"])[0, k % 3] = v
            assert _check(q) == (T.TRT_ERR_INVALID, 0), (v, k)
    many = np.concatenate([_pt()] * 9)  # the lowest bad index, whichever part of the predicate fails
    many["tmax"][7] = np.nan
    many["pos"][4, 1] = np.nan
    many["n"][8, 2] = np.inf
    assert _check(many) == (T.TRT_ERR_INVALID, 4)
    many["pos"][4, 1] = 0
    assert _check(many) == (T.TRT_ERR_INVALID, 7)
    many["tmax"][7] = 2.0
    assert _check(many) == (T.TRT_ERR_INVALID, 8)
    many["n"][8] = (0, 1, 0)
    assert _check(many) == (0, 0)


# ---- trt_point_segments against a float32 numpy restatement -----------------------------------------


def restated(points, mode, e):
    """abi.h's segment (i, k) in float32 numpy, every product and sum rounded on its own."""
    p = np.ascontiguousarray(points, T.QPOINT).reshape(-1)
    e = np.asarray(e, f32)[:, :3]
    out = np.zeros((len(p), len(e)), T.QSEG)
    pos, n = p["pos"][:, None, :], p["n"][:, None, :]
    out["org"] = np.broadcast_to(pos, out["org"].shape)
    if mode == T.VIS_DIRS:
        ee = np.broadcast_to(e[None], out["dir"].shape)
        with np.errstate(over="ignore", invalid="ignore"):
            s = (ee[..., 0] * n[..., 0] + ee[..., 1] * n[..., 1]) + ee[..., 2] * n[..., 2]
        out["dir"] = np.where((s < 0)[..., None], -ee, ee)
        out["tmax"] = p["tmax"][:, None]
    else:
        with np.errstate(over="ignore"):
            d = (e[None] - pos).astype(f32)
            x, y, z = d[..., 0], d[..., 1], d[..., 2]
            length = np.sqrt((x * x + y * y) + z * z, dtype=f32)
        out["dir"] = d
        out["tmax"] = np.minimum(length, p["tmax"][:, None])
    return out


def _points(n, seed, tmax):
    rays = random_rays(n, seed)
    p = np.zeros(n, T.QPOINT)
    p["pos"], p["n"], p["tmax"] = rays["org"], rays["dir"], tmax
    return p


def test_point_segments_dirs_equal_the_restatement():
    p = _points(300, 3, np.random.default_rng(1).uniform(0.1, 50.0, 300).astype(f32))
    for k in (1, 5, 16, 63):
        dirs = S.sphere_dirs(k)
        got = S.point_segments(p, dirs=dirs)
        assert got.dtype == T.QSEG and got.shape == (300, k)
        want = restated(p, T.VIS_DIRS, dirs)
        assert got.tobytes() == want.tobytes(), k
        flipped = (got["dir"] != dirs[None]).any(-1)
        assert k == 1 or (flipped.any() and not flipped.all())
        assert lib().trt_check_segs(got.ctypes.data, got.size, None) == 0
    # a fourth column is carried and ignored
    four = np.concatenate([S.sphere_dirs(7), np.full((7, 1), np.nan, f32)], 1)
    assert S.point_segments(p, dirs=four).tobytes() == S.point_segments(p, dirs=four[:, :3]).tobytes()


def test_point_segments_flip_cases():
    e = np.array([[1.0, 2.0, -3.0], [0.5, 0.0, 0.0]], f32)
    cases = {
        "s = +0": ((0.0, 3.0, 2.0), False),        # 1*0 + 2*3 + -3*2 = +0 for entry 0
        "s = -0": ((-0.0, -0.0, 0.0), False),      # 1*-0 + 2*-0 + -3*0: three products of -0.0, s = -0.0
        "n = 0": ((0.0, 0.0, 0.0), False),
        "s tiny negative": ((-1e-38, 0.0, 0.0), True),   # 1 * -1e-38: a subnormal-range negative
        "s negative": ((-1.0, -1.0, 0.0), True),
        "s positive": ((1.0, 1.0, 0.0), False),
    }
    for name, (n, flip) in cases.items():
        q = _pt(n=n, tmax=2.5)
        got = S.point_segments(q, dirs=e)
        assert got.tobytes() == restated(q, T.VIS_DIRS, e).tobytes(), name
        want0 = -e[0] if flip else e[0]
        assert got["dir"][0, 0].tobytes() == want0.tobytes(), name
        assert (got["tmax"] == f32(2.5)).all() and (got["org"] == q["pos"][0]).all() and not got["pad"].any()
    with np.errstate(under="ignore"):
        s = f32(1.0) * f32(-1e-38)
    assert s < 0 and abs(s) < np.finfo(f32).tiny * 2
    tiny = _pt(n=(-float(TINY), 0.0, 0.0))  # s = -1.4e-45, the smallest negative there is: still a flip
    assert S.point_segments(tiny, dirs=e)["dir"][0, 0].tobytes() == (-e[0]).tobytes()


def test_point_segments_targets():
    rng = np.random.default_rng(8)
    p = _points(400, 11, rng.choice([0.5, 3.0, 20.0, 1e10], 400).astype(f32))
    targets = np.array([[-20, 20, 20], [30, 50, -25], [30, 20, 30], [0.5, 0.25, -7.0]], f32)
    got = S.point_segments(p, targets=targets)
    assert got.shape == (400, 4)
    assert got.tobytes() == restated(p, T.VIS_TARGETS, targets).tobytes()
    between = S.segments_between(p["pos"][:, None, :], targets[None])
    assert got["dir"].tobytes() == between["dir"].tobytes() and got["org"].tobytes() == between["org"].tobytes()
    assert got["tmax"].tobytes() == np.minimum(between["tmax"], p["tmax"][:, None]).tobytes()
    capped = got["tmax"] < between["tmax"]
    assert capped.any() and not capped.all()  # the point's tmax is a range cap
    assert lib().trt_check_segs(got.ctypes.data, got.size, None) == 0


def test_point_on_its_target_gives_a_record_check_segs_rejects():
    q = np.concatenate([_pt(pos=(1.0, 2.0, 3.0)), _pt(pos=(-20.0, 20.0, 20.0)), _pt(pos=(0.0, 0.0, 0.0))])
    targets = np.array([[5, 5, 5], [-20, 20, 20]], f32)
    got = S.point_segments(q, targets=targets)
    assert got.tobytes() == restated(q, T.VIS_TARGETS, targets).tobytes()
    assert (got["dir"][1, 1] == 0).all() and got["tmax"][1, 1] == 0  # emitted as computed
    bad = ctypes.c_uint32(0xDEAD)
    flat = got.reshape(-1)
    assert lib().trt_check_segs(flat.ctypes.data, len(flat), ctypes.byref(bad)) == T.TRT_ERR_INVALID
    assert bad.value == 1 * 2 + 1  # out[i * nset + k]
    for i in (0, 1, 2, 4, 5):
        assert lib().trt_check_segs(flat[i:i + 1].ctypes.data, 1, None) == 0, i


def _segments_rc(p, e, mode, nset=None):
    p = np.ascontiguousarray(p, T.QPOINT).reshape(-1)
    e = np.ascontiguousarray(e, f32)
    nset = len(e) if nset is None else nset
    out = np.zeros(max(1, len(p) * max(nset, 1)), T.QSEG)
    return lib().trt_point_segments(p.ctypes.data, len(p), e.ctypes.data, nset, mode, out.ctypes.data)


def test_point_segments_refusals():
    p = _points(3, 2, 1.0)
    e = np.zeros((64, 4), f32)
    e[:, 1] = 1.0
    assert _segments_rc(p, e[:63], T.VIS_DIRS) == 0
    assert _segments_rc(p, e, T.VIS_DIRS, nset=0) == T.TRT_ERR_INVALID
    assert _segments_rc(p, e, T.VIS_DIRS, nset=64) == T.TRT_ERR_INVALID
    assert _segments_rc(p, e, T.VIS_TARGETS, nset=64) == T.TRT_ERR_INVALID
    assert _segments_rc(p, e[:4], 2) == T.TRT_ERR_INVALID  # an unknown mode
    out = np.zeros(12, T.QSEG)
    assert lib().trt_point_segments(None, 3, e.ctypes.data, 4, T.VIS_DIRS, out.ctypes.data) == T.TRT_ERR_INVALID
    assert lib().trt_point_segments(p.ctypes.data, 3, None, 4, T.VIS_DIRS, out.ctypes.data) == T.TRT_ERR_INVALID
    assert lib().trt_point_segments(p.ctypes.data, 3, e.ctypes.data, 4, T.VIS_DIRS, None) == T.TRT_ERR_INVALID
    badp = p.copy()
    badp["tmax"][1] = 0
    assert _segments_rc(badp, e[:4], T.VIS_DIRS) == T.TRT_ERR_INVALID
    # set entries: a DIRS entry is a valid ray direction, a TARGETS entry is finite
    z = e[:4].copy()
    z[2, :3] = 0
    assert _segments_rc(p, z, T.VIS_DIRS) == T.TRT_ERR_INVALID
    assert _segments_rc(p, z, T.VIS_TARGETS) == 0  # the origin is a fine target
    for v, both in ((np.nan, True), (np.inf, True), (1e16, False), (1e-16, False)):
        w = np.zeros((2, 4), f32)
        w[0, 1] = 1.0
        w[1, 0] = v
        assert _segments_rc(p, w, T.VIS_DIRS) == T.TRT_ERR_INVALID, v
        assert (_segments_rc(p, w, T.VIS_TARGETS) == T.TRT_ERR_INVALID) == both, v
    with pytest.raises(TrtError):
        S.point_segments(p, dirs=z)
    with pytest.raises(ValueError):
        S.point_segments(p)
    with pytest.raises(ValueError):
        S.point_segments(p, dirs=e[:3], targets=e[:3])
    with pytest.raises(ValueError):
        S.point_segments(p, dirs=np.zeros((3, 2)))


# ---- the scene module's helpers ----------------------------------------------------------------------


def test_sphere_dirs():
    for k in (1, 2, 16, 63):
        d = S.sphere_dirs(k)
        assert d.dtype == f32 and d.shape == (k, 3)
        # float64 unit vectors rounded once: each component is off by at most half an ulp, a relative
        # 2^-24, so the length is within 2^-24 of 1 — inside one ulp of 1.0 (2^-23)
        norm = np.sqrt((d.astype(np.float64) ** 2).sum(1))
        assert np.abs(norm - 1.0).max() <= 2.0 ** -23, k
        assert S.point_segments(_pt(), dirs=d).shape == (1, k)  # every one is a valid set entry
    d = S.sphere_dirs(63)
    assert d[0] @ d[-1] < -0.9 and d[0, 1] > 0.9 and d[-1, 1] < -0.9  # first and last on opposite sides
    assert len(np.unique(d, axis=0)) == 63
    assert abs(d.astype(np.float64).mean(0)).max() < 0.05  # spread over the sphere: the mean is near the centre
    with pytest.raises(ValueError):
        S.sphere_dirs(0)


def test_points_on_hits():
    rays = random_rays(6, 1)
    hits = np.zeros(6, T.QHIT)
    hits["kind"] = (T.HIT_FLOOR, T.HIT_NONE, T.HIT_SPHERE, T.HIT_TRIANGLE, T.HIT_BAD_RAY, T.HIT_FLOOR)
    hits["t"] = (2.0, 1e10, 3.5, 0.25, 0.0, 7.0)
    rays["dir"][0] = (0.0, -2.0, 0.0)  # onto the floor from above: the normal already faces the ray
    rays["dir"][5] = (0.0, 3.0, 0.0)   # from below: turned
    hits["n"][[0, 5]] = (0.0, 1.0, 0.0)
    hits["n"][2] = (0.6, 0.0, 0.8)
    hits["n"][3] = (0.0, 0.0, -1.0)
    pts, idx = S.points_on_hits(rays, hits, offset=0.5, tmax=2.0)
    assert pts.dtype == T.QPOINT and idx.tolist() == [0, 2, 3, 5]
    assert (pts["tmax"] == f32(2.0)).all() and not pts["pad"].any() and _check(pts) == (0, 0)
    o = rays["org"].astype(np.float64)
    assert pts["n"][0].tolist() == [0.0, 1.0, 0.0] and pts["n"][3].tolist() == [0.0, -1.0, 0.0]
    assert pts["pos"][0].tobytes() == (o[0] + 2.0 * np.array((0, -1.0, 0)) + 0.5 * np.array((0, 1.0, 0))).astype(f32).tobytes()
    assert pts["pos"][3].tobytes() == (o[5] + 7.0 * np.array((0, 1.0, 0)) + 0.5 * np.array((0, -1.0, 0))).astype(f32).tobytes()
    for j, i in ((1, 2), (2, 3)):
        d = rays["dir"][i].astype(np.float64)
        d /= np.sqrt((d * d).sum())
        n = hits["n"][i].astype(np.float64)
        n = -n if n @ d > 0 else n
        assert pts["n"][j].tobytes() == n.astype(f32).tobytes()
        assert pts["pos"][j].tobytes() == (o[i] + float(hits["t"][i]) * d + 0.5 * n).astype(f32).tobytes()
    default, _ = S.points_on_hits(rays, hits)
    assert (default["tmax"] == T.QSEG_MAX_T).all()
