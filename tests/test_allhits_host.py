"""The host side of the all-hits queries (abi.h trt_trace_all): the ABI additions, the argument
refusals that need no device, the properties of the reference the GPU tests compare against
(tests/allhits_common.py) and the numpy helpers of the scene module.  No GPU."""
from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import allhits_common as AH
from tests.occlusion_common import expected_occluded
from tests.query_common import random_rays
from vkcomputeshader_tinyraytracer_amd import ABI_SYMBOLS, LIB_PATH, lib, scene as S, types as T

f32 = np.float32
REPO = Path(__file__).resolve().parents[1]
HEADER = (REPO / "include" / "trt" / "abi.h").read_text()


def test_symbol_and_constants():
    from vkcomputeshader_tinyraytracer_amd._lib import ABI_VERSION

    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (trt_\w+)", out))
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert "trt_trace_all" in exported and "trt_trace_all" in ABI_SYMBOLS and hasattr(lib(), "trt_trace_all")
    assert re.search(r"\bint trt_trace_all\s*\(", code)
    assert ABI_VERSION == 5 and "#define TRT_ABI_VERSION 5\n" in HEADER
    for name, val in (("TRT_ALLHITS_MAX", "32u"), ("TRT_ALLHITS_MORE", "0x80000000u"), ("TRT_ALLHITS_BAD_SEG", "0xffffffffu")):
        assert re.search(rf"#define {name} +{val}(\s|$)", HEADER, flags=re.M), name
    assert (T.ALLHITS_MAX, T.ALLHITS_MORE, T.ALLHITS_BAD_SEG) == (32, 0x80000000, 0xFFFFFFFF)
    assert b"all_hits_kernel" in LIB_PATH.read_bytes()  # the kernel is in the code object
    import vkcomputeshader_tinyraytracer_amd as trt

    assert trt.inside_length is S.inside_length and trt.crossing_parity is S.crossing_parity
    assert callable(trt.Renderer.trace_all) and callable(trt.Renderer.contains)


def test_refusals_that_need_no_device():
    L = lib()
    p = T.Params()
    L.trt_params_default(ctypes.byref(p))
    segs = S.segments_from_rays(random_rays(4, 1))
    counts = np.zeros(4, np.uint32)
    # a null context is refused before anything is read
    assert L.trt_trace_all(None, ctypes.byref(p), segs.ctypes.data, 4, 8, None, counts.ctypes.data, None) == T.TRT_ERR_INVALID
    assert L.trt_trace_all(None, None, None, 0, 0, None, None, None) == T.TRT_ERR_INVALID
    assert not counts.any()


# ---- the reference's own properties ----------------------------------------------------------------


@pytest.fixture(scope="module")
def ref():
    sc = S.config_c3(71, 41, env_size=(64, 32), level=2)
    rays = random_rays(60, 77)
    rng = np.random.default_rng(3)
    aim = np.arange(0, len(rays), 2)  # every second ray through the icosphere: several crossings
    rays["org"][aim] = (np.array((2.5, -2.0, -10.0)) + rng.uniform(-4, 4, size=(len(aim), 3))).astype(f32)
    rays["dir"][aim] = (np.array((2.5, -2.0, -10.0)) + rng.uniform(-1.0, 1.0, size=(len(aim), 3)) - rays["org"][aim]).astype(f32)
    segs = S.segments_from_rays(rays)
    cands = AH.all_candidates(sc, segs, sc.flags)
    return sc, segs, cands


def test_reference_order_and_prefix(ref):
    sc, segs, cands = ref
    tot = AH.totals(cands)
    assert tot.max() >= 3 and (tot == 0).any()
    for c in cands:
        keys = [r[:4] for r in c]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        assert all(r[0] > AH.EPS for r in c)
    h32, c32 = AH.expected_all_hits(sc, segs, sc.flags, 32, cands)
    assert not (c32 & T.ALLHITS_MORE).any() and (c32 == tot).all()
    for k in (1, 2, 4):
        hk, ck = AH.expected_all_hits(sc, segs, sc.flags, k, cands)
        assert hk.tobytes() == np.ascontiguousarray(h32[:, :k]).tobytes()
        assert ((ck & 0x7FFFFFFF) == np.minimum(tot, k)).all()
        assert (((ck & T.ALLHITS_MORE) != 0) == (tot > k)).all()
    # slots past the count are the miss record
    past = np.arange(32)[None, :] >= tot[:, None]
    assert h32[past].tobytes() == np.tile(AH.MISS, int(past.sum())).tobytes()


def test_reference_tmax_is_strict_and_counts_agree_with_occlusion(ref):
    sc, segs, cands = ref
    tot = AH.totals(cands)
    h32, _ = AH.records(cands, 32)
    # cut every segment off at the t of its record j: exactly the records with a smaller t remain
    cut, which = [], []
    for i in np.flatnonzero(tot >= 2):
        for j in (1, int(tot[i]) - 1):
            s = segs[i:i + 1].copy()
            s["tmax"] = h32[i, j]["t"]
            cut.append(s)
            which.append((i, j))
    cut = np.concatenate(cut)
    got = AH.all_candidates(sc, cut, sc.flags)
    for (i, j), c in zip(which, got):
        want = [r for r in cands[i] if r[0] < h32[i, j]["t"]]
        assert [r[:4] for r in c] == [r[:4] for r in want]
        assert len(c) <= j
    for flags in (int(sc.flags), int(sc.flags) & ~T.FLAG_FLOOR):
        c = cands if flags == int(sc.flags) else AH.all_candidates(sc, segs, flags)
        occ = expected_occluded(sc, segs, flags)
        assert ((AH.totals(c) > 0) == (occ == T.OCC_OCCLUDED)).all()
        if flags != int(sc.flags):
            assert not any(r[4] == T.HIT_FLOOR for cc in c for r in cc)
            assert any(r[4] == T.HIT_FLOOR for cc in cands for r in cc)


def test_sphere_roots_give_an_entry_and_an_exit():
    sc = S.config_c2(71, 41, env_size=(64, 32))
    segs = np.zeros(3, T.QSEG)
    cr = np.asarray(sc.ubo["sphere0"]["center_radius"], f32).reshape(4)
    segs["org"][0] = cr[:3] + np.array((0, 0, 10), f32)  # from outside, through the centre
    segs["dir"][0] = (0, 0, -1)
    segs["org"][1] = cr[:3]                                # from the centre: the exit only
    segs["dir"][1] = (0, 0, -1)
    segs["org"][2] = cr[:3] + np.array((0, 0, 10), f32)  # cut off inside the sphere: the entry only
    segs["dir"][2] = (0, 0, -1)
    segs["tmax"] = (1e10, 1e10, 10.0)
    flags = int(sc.flags) & ~T.FLAG_FLOOR
    c = AH.all_candidates(sc, segs, flags)
    mine = [[r for r in cc if r[4] == T.HIT_SPHERE and r[5] == 0] for cc in c]
    assert [len(m) for m in mine] == [2, 1, 1]
    assert mine[0][0][0] == f32(10) - cr[3] and mine[0][1][0] == f32(10) + cr[3]
    assert mine[1][0][0] == cr[3] and mine[2][0][0] == f32(10) - cr[3]


# ---- the scene module's helpers ---------------------------------------------------------------------


def _rec(*slots, k=6):
    h = np.tile(AH.MISS, (1, k))
    for j, (kind, t) in enumerate(slots):
        h[0, j]["kind"], h[0, j]["t"] = kind, t
    return h


def test_inside_length():
    TRI, SPH, FLO = T.HIT_TRIANGLE, T.HIT_SPHERE, T.HIT_FLOOR
    rows = [
        (_rec((TRI, 1.0), (TRI, 3.5)), 2, 2.5),
        (_rec((TRI, 1.0), (TRI, 3.5), (TRI, 4.0), (TRI, 4.25)), 4, 2.75),
        (_rec((TRI, 1.0), (TRI, 3.5), (TRI, 4.0)), 3, 2.5),                  # an unpaired last crossing
        (_rec((SPH, 0.5), (TRI, 1.0), (FLO, 2.0), (TRI, 3.0), (SPH, 9.0)), 5, 2.0),  # other kinds are left out
        (_rec(), 0, 0.0),
        (_rec((TRI, 1.0), (TRI, 3.5), (TRI, 4.0), (TRI, 4.25)), 2 | T.ALLHITS_MORE, 2.5),  # the count bounds the records
        (_rec((TRI, 1.0), (TRI, 3.5)), T.ALLHITS_BAD_SEG, 0.0),
    ]
    hits = np.concatenate([r[0] for r in rows])
    counts = np.array([r[1] for r in rows], np.uint32)
    got = S.inside_length(hits, counts)
    assert got.dtype == np.float64 and got.tolist() == [r[2] for r in rows]
    assert S.inside_length(hits, counts.view(np.int32)).tolist() == got.tolist()  # a device query's int32 bits
    with pytest.raises(ValueError):
        S.inside_length(hits, counts[:3])


def test_crossing_parity():
    counts = np.array([0, 1, 2, 3, 32, 32 | T.ALLHITS_MORE, 5 | T.ALLHITS_MORE, T.ALLHITS_BAD_SEG], np.uint32)
    odd, trunc = S.crossing_parity(counts)
    assert odd.dtype == bool and trunc.dtype == bool
    assert odd.tolist() == [False, True, False, True, False, False, True, False]
    assert trunc.tolist() == [False, False, False, False, False, True, True, True]
    o2, t2 = S.crossing_parity(counts.view(np.int32))
    assert o2.tolist() == odd.tolist() and t2.tolist() == trunc.tolist()
