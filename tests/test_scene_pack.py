"""The host packing of a scene (csrc/scene_pack.cpp pack_scene, through trt_diag_scene_pack, no
GPU): what trt_upload_scene copies to the device, pinned byte for byte.  Every adversarial mesh of
tests/mesh_cases.py (NaN vertices, inverted batch boxes, degenerate triangles, deep hierarchies),
the deep-stack meshes, every mesh of tests/golden/meshes.npz and the empty scene are packed, and
`top`, `node_off` and each array's element count and 64-bit FNV-1a hash are compared with
tests/golden/scene_pack_hashes.json, which was recorded when the packing was cut out of
trt_upload_scene unchanged.

A case takes what the host BVH build of its mesh takes: milliseconds for the adversarial meshes,
0.2 to 1.0 s for the golden ones (venus, the largest, 1.0 s; the diagnostic returns the collapse's
stack too, so that no case builds its hierarchy twice).

TRT_RECORD_SCENE_PACK=1 rewrites the golden file instead of comparing (only for a change that is
meant to change the packing)."""
from __future__ import annotations

import ctypes
import json
import os
from pathlib import Path

import numpy as np
import pytest

from tests import mesh_cases as M
from vkcomputeshader_tinyraytracer_amd import lib, scene as S, types as T

GOLDEN = Path(__file__).resolve().parent / "golden" / "scene_pack_hashes.json"
ARRAYS = ("batches", "nodes", "geo", "shade", "mats", "bvh", "bvh4", "bvh4q", "bvh_tris")

_MESHES = S.load_golden_meshes()
_DEEP_SCENES = {d.scene.name: d.scene for d in M.DEEP.values()}  # the cameras differ, the meshes do not


def _arrays(name):
    if name == "empty":
        return np.zeros(0, T.TRIANGLE), np.zeros(0, T.MODEL)
    if name.startswith("golden:"):
        return S.build_models([name[7:]], _MESHES)
    sc = M.CASES[name].scene if name in M.CASES else _DEEP_SCENES[name]
    return np.ascontiguousarray(sc.tris, T.TRIANGLE), np.ascontiguousarray(sc.models, T.MODEL)


NAMES = (["empty"] + sorted(M.CASES) + sorted(_DEEP_SCENES) +
         ["golden:" + n for n in sorted(S.MODEL_INFOS) if S.MODEL_INFOS[n].asset + ":pos" in _MESHES])


def pack(tris, models) -> tuple:
    f = lib().trt_diag_scene_pack
    out = (ctypes.c_uint64 * 31)()
    assert f(tris.ctypes.data, len(tris), models.ctypes.data, len(models), out) == 0
    v = [int(x) for x in out]
    d = {"top": v[0], "node_off": v[1:12]}
    for i, a in enumerate(ARRAYS):
        d[a] = [v[12 + 2 * i], f"{v[13 + 2 * i]:016x}"]
    return d, v[30]


def test_the_golden_file_lists_these_cases():
    if os.environ.get("TRT_RECORD_SCENE_PACK") == "1":
        GOLDEN.write_text(json.dumps({n: pack(*_arrays(n))[0] for n in NAMES}, indent=1, sort_keys=True) + "\n")
    assert sorted(json.loads(GOLDEN.read_text())) == sorted(NAMES)
    assert "fan_overflow" in NAMES and any(n.startswith("golden:") for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_pack_scene_is_the_recorded_one(name):
    tris, models = _arrays(name)
    got, stack = pack(tris, models)
    assert got == json.loads(GOLDEN.read_text())[name]
    # what the upload relies on: one record per batch and triangle, at least one material
    assert got["batches"][0] == len(models) and got["geo"][0] == got["shade"][0] == len(tris)
    assert got["mats"][0] >= 1 and got["nodes"][0] % 2 == 0
    # the 4-wide nodes are dropped exactly when the collapse's stack exceeds kBvhStack, and there
    # are no quantized nodes without them
    if got["bvh"][0] == 0:  # no BVH is built: the batch walk traces the scene
        assert got["bvh4"][0] == got["bvh4q"][0] == got["bvh_tris"][0] == stack == 0
        return
    assert got["bvh_tris"][0] >= len(tris) and stack >= 1
    assert (got["bvh4"][0] == 0) == (stack > M.K_BVH_STACK), stack
    assert got["bvh4q"][0] in (0, got["bvh4"][0])
    if name in M.CASES:  # the case is there for its walk
        assert M.CASES[name].bvh and (got["bvh4"][0] == 0) == M.CASES[name].fallback
