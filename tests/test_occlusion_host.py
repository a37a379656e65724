"""The host side of the occlusion queries (abi.h trt_occluded): the ABI additions, the shared segment
predicate behind trt_check_segs, and the segment helpers of the scene module.  No GPU."""
from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.occlusion_common import boundary_segments, expected_occluded, hits_for
from tests.query_common import random_rays
from vkcomputeshader_tinyraytracer_amd import ABI_SYMBOLS, LIB_PATH, lib, scene as S, types as T

f32 = np.float32
REPO = Path(__file__).resolve().parents[1]
HEADER = (REPO / "include" / "trt" / "abi.h").read_text()


def test_sizes_and_constants():
    m = re.search(r"typedef struct trt_qseg \{([^}]*)\} trt_qseg;", HEADER)
    assert m, "trt_qseg is not declared"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "float org[3]; float tmax; float dir[3]; float pad;"
    assert "static_assert(sizeof(trt_qseg) == 32" in HEADER
    assert T.QSEG.itemsize == 32
    assert {n: T.QSEG.fields[n][1] for n in T.QSEG.names} == {"org": 0, "tmax": 12, "dir": 16, "pad": 28}
    assert all(T.QSEG.fields[n][0].base == np.dtype("<f4") for n in T.QSEG.names)
    for name, val in (("TRT_OCC_VISIBLE", "0u"), ("TRT_OCC_OCCLUDED", "1u"), ("TRT_OCC_BAD_SEG", "0xffu"),
                      ("TRT_QSEG_MAX_T", "1e10f")):
        assert re.search(rf"#define {name} +{val}(\s|$)", HEADER, flags=re.M), name
    assert (T.OCC_VISIBLE, T.OCC_OCCLUDED, T.OCC_BAD_SEG) == (0, 1, 0xFF)
    assert isinstance(T.QSEG_MAX_T, f32) and T.QSEG_MAX_T == f32(1e10)


def test_exports_and_version():
    from vkcomputeshader_tinyraytracer_amd._lib import ABI_VERSION

    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (trt_\w+)", out))
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("trt_occluded", "trt_check_segs"):
        assert name in exported and name in ABI_SYMBOLS and hasattr(lib(), name)
        assert re.search(rf"\bint {name}\s*\(", code), name
    assert ABI_VERSION == 5 and "#define TRT_ABI_VERSION 5\n" in HEADER
    assert b"occlusion_query_kernel" in LIB_PATH.read_bytes()  # the kernel is in the code object


def _check(segs):
    s = np.ascontiguousarray(segs, T.QSEG).reshape(-1)
    bad = ctypes.c_uint32(0xDEAD)
    rc = lib().trt_check_segs(s.ctypes.data if len(s) else None, len(s), ctypes.byref(bad))
    return rc, bad.value


def _seg(org=(0.5, 1.0, -2.0), d=(0.0, 0.0, -1.0), tmax=3.0):
    q = np.zeros(1, T.QSEG)
    q["org"], q["dir"], q["tmax"] = org, d, tmax
    return q


TINY = np.nextafter(f32(0), f32(1))  # the smallest positive subnormal


def test_check_segs_valid_edges():
    assert _check(np.zeros(0, T.QSEG)) == (0, 0)
    assert TINY > 0 and TINY == f32(1.4e-45)
    for tmax in (TINY, f32(1e-4), f32(1e10), f32(1.0)):
        assert _check(_seg(tmax=tmax)) == (0, 0), tmax
    for length in (1.0, 1e-3, 1e3):  # the kernel normalizes: any ordinary length is accepted
        assert _check(_seg(d=(0.6 * length, 0.0, -0.8 * length)))[0] == 0, length


def test_check_segs_invalid_edges():
    assert lib().trt_check_segs(None, 3, None) == T.TRT_ERR_INVALID
    bad = ctypes.c_uint32(0xDEAD)
    assert lib().trt_check_segs(None, 3, ctypes.byref(bad)) == T.TRT_ERR_INVALID and bad.value == 0
    over = np.nextafter(f32(1e10), f32(np.inf))
    assert over > f32(1e10)
    for tmax in (f32(0.0), f32(-0.0), f32(-1.0), over, f32(np.inf), f32(-np.inf), f32(np.nan)):
        assert _check(_seg(tmax=tmax)) == (T.TRT_ERR_INVALID, 0), tmax
    # every case trt_check_rays rejects (tests/test_query_host.py::test_check_rays)
    for v in (float("nan"), float("inf"), -float("inf")):
        for k in range(6):
            q = _seg(d=(0.1, 0.2, -1.0))
            (q["org"] if k < 3 else q["dir"])[0, k % 3] = v
            assert _check(q)[0] == T.TRT_ERR_INVALID, (v, k)
    for d in ((0.0, 0.0, 0.0), (0.0, 1e-16, 0.0), (0.0, 0.0, 1e16), (3e19, 0.0, 0.0)):
        assert _check(_seg(d=d))[0] == T.TRT_ERR_INVALID, d
    # the lowest bad index, whichever part of the predicate fails there
    many = np.concatenate([_seg()] * 9)
    many["tmax"][7] = np.nan
    many["org"][4, 1] = np.nan
    many["dir"][8] = 0
    assert _check(many) == (T.TRT_ERR_INVALID, 4)
    many["org"][4, 1] = 0
    assert _check(many) == (T.TRT_ERR_INVALID, 7)
    many["tmax"][7] = 2.0
    assert _check(many) == (T.TRT_ERR_INVALID, 8)
    many["dir"][8] = (0, 1, 0)
    assert _check(many) == (0, 0)


def test_check_segs_agrees_with_check_rays_and_the_tmax_range_on_random_bits():
    rng = np.random.default_rng(20261)
    n = 6000
    s = np.zeros(n, T.QSEG)
    bits = rng.integers(0, 2**32, size=(n, 7), dtype=np.uint64).astype(np.uint32)
    tame = rng.random((n, 7)) < 0.8
    bits = np.where(tame, (bits & np.uint32(0x807FFFFF)) | (rng.integers(90, 165, size=(n, 7)).astype(np.uint32) << 23), bits)
    fl = bits.view(f32)
    s["org"], s["dir"], s["tmax"] = fl[:, :3], fl[:, 3:6], fl[:, 6]
    L = lib()
    rays = np.zeros(n, T.QRAY)
    rays["org"], rays["dir"] = s["org"], s["dir"]
    ray_ok = np.array([L.trt_check_rays(rays[i:i + 1].ctypes.data, 1, None) == 0 for i in range(n)])
    with np.errstate(invalid="ignore"):
        want = ray_ok & (s["tmax"] > 0) & (s["tmax"] <= T.QSEG_MAX_T)
    assert 0.1 < want.mean() < 0.9 and (ray_ok & ~want).any() and (~ray_ok).any()
    got = np.array([L.trt_check_segs(s[i:i + 1].ctypes.data, 1, None) == 0 for i in range(n)])
    assert np.array_equal(got, want)
    assert _check(s) == (T.TRT_ERR_INVALID, int(np.argmin(want)))


def _ulp(x):
    x = np.abs(np.asarray(x, f32))
    return (np.nextafter(x, f32(np.inf)) - x).astype(np.float64)


def test_segments_between():
    rng = np.random.default_rng(5)
    n = 4000
    a = rng.uniform((-8, -3, -28), (8, 6, 2), size=(n, 3)).astype(f32)
    b = (a.astype(np.float64) + rng.normal(size=(n, 3)) * rng.choice([1e-3, 0.1, 3.0, 40.0], size=(n, 1))).astype(f32)
    s = S.segments_between(a, b)
    assert s.dtype == T.QSEG and s.shape == (n,)
    d64 = b.astype(np.float64) - a.astype(np.float64)
    assert s["org"].tobytes() == a.tobytes()
    assert s["dir"].tobytes() == d64.astype(f32).tobytes()  # a float32 difference is the rounded exact one
    # the length against float64 over the stored direction: within 1 ulp, counted as float32
    # steps between tmax and the float64 length rounded to float32 (both are float32 values, so
    # the distance is a whole number of steps).  The float32 chain the kernel shares (three
    # rounded products and sums, then a rounded square root) carries up to about 2 ulp of real
    # error in the worst case; on this sample the real error reaches 1.09 ulp (printed), which
    # is one step from the correctly rounded length.
    ref = np.sqrt((s["dir"].astype(np.float64) ** 2).sum(-1))
    real = np.abs(s["tmax"].astype(np.float64) - ref) / _ulp(ref.astype(f32))
    steps = np.abs(s["tmax"].view(np.int32).astype(np.int64) - ref.astype(f32).view(np.int32).astype(np.int64))
    print(f"segments_between: tmax vs float64: max {steps.max()} float32 steps, real error max {real.max():.3f} ulp")
    assert steps.max() <= 1
    # and it is the project's dot order, bit for bit
    x, y, z = (s["dir"][:, k] for k in range(3))
    assert s["tmax"].tobytes() == np.sqrt((x * x + y * y) + z * z).astype(f32).tobytes()
    assert not s["pad"].any() and _check(s) == (0, 0)
    # broadcasting: many origins, one target
    one = S.segments_between(a[:5], (1.0, 2.0, 3.0))
    assert one.shape == (5,) and (one["dir"] == (np.array((1, 2, 3), f32) - a[:5])).all()
    with pytest.raises(ValueError):
        S.segments_between(np.zeros((3, 2)), np.zeros((3, 2)))


def test_segments_from_rays():
    rays = random_rays(7, 1).reshape(7)
    s = S.segments_from_rays(rays)
    assert s.dtype == T.QSEG and s["org"].tobytes() == rays["org"].tobytes() and s["dir"].tobytes() == rays["dir"].tobytes()
    assert (s["tmax"] == T.QSEG_MAX_T).all() and not s["pad"].any()
    t = np.arange(1, 8, dtype=f32)
    assert (S.segments_from_rays(rays, t)["tmax"] == t).all()
    assert (S.segments_from_rays(rays, 2.5)["tmax"] == f32(2.5)).all()


def test_expected_occluded_is_the_identity_on_the_oracle():
    """The reference of the GPU tests on a handful of rays: strict at t, occluded just beyond it,
    and without the floor flag the floor hits drop out."""
    sc = S.config_c2(71, 41, env_size=(64, 32))
    rays = random_rays(40, 77)
    hits = hits_for(sc, rays, sc.flags)
    assert (hits["kind"] == T.HIT_FLOOR).any() and (hits["kind"] == T.HIT_NONE).any()
    segs, idx = boundary_segments(rays, hits)
    want = expected_occluded(sc, segs, sc.flags, hits[idx])
    assert want.tobytes() == expected_occluded(sc, segs, sc.flags).tobytes()
    hit = hits["kind"][idx] != T.HIT_NONE
    assert (want[~hit] == T.OCC_VISIBLE).all()
    assert want[hit].reshape(-1, 3)[:, 0].tolist() == [T.OCC_VISIBLE] * (hit.sum() // 3)
    assert want[hit].reshape(-1, 3)[:, 1].tolist() == [T.OCC_OCCLUDED] * (hit.sum() // 3)
    off = expected_occluded(sc, segs, sc.flags & ~T.FLAG_FLOOR)
    floor = hits["kind"][idx] == T.HIT_FLOOR
    # nothing else is as near as the floor was, so those segments are now clear
    assert floor.any() and (off[floor] == T.OCC_VISIBLE).all() and (want[floor] == T.OCC_OCCLUDED).any()
    assert off[~floor].tobytes() == want[~floor].tobytes()
