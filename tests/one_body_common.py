"""Shared by tests/test_gpu_one_body.py and the recording of tests/golden/one_body_parent_hashes.json:
the cases, the contexts and the frames whose hashes the golden file holds."""
from __future__ import annotations

import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from vkcomputeshader_tinyraytracer_amd import Renderer, scene as S, types as T

ENV = (64, 32)
SPEED = 0.5  # per frame: the horizon, the floor's edges and the shadow outlines cross 8x8 tiles within a pair
SIZES = [(128, 96), (100, 52)]
DEPTHS = [1, 2, 3, 4, 5, 8]  # CAP 0 ... 4 and the kernel with the private stack
# a single frame, a whole pair, an odd last pair, and a span-table boundary (16 frames per table)
# inside the launch, before a whole pair and before an odd one
COUNTS = [1, 2, 3, 16, 17, 33]
NMAX = max(COUNTS)
KNOBS = ("TRT_SKY_TABLE", "TRT_SKY_SPANS", "TRT_SKY_SPAN_FRAMES", "TRT_SHADOW_MASK", "TRT_SHADOW_MASK_CELL",
         "TRT_FLOOR_CLASS")
# default: sky_trace_kernel_floor, then _smask, sky_trace_kernel, _nospan, and trace_kernel
OFF = ("TRT_FLOOR_CLASS", "TRT_SHADOW_MASK", "TRT_SKY_SPANS", "TRT_SKY_TABLE")
NAMES = ("default",) + tuple(k + "=0" for k in OFF)
GOLDEN = Path(__file__).resolve().parent / "golden" / "one_body_parent_hashes.json"


def contexts(device):
    """(default, TRT_FLOOR_CLASS=0, TRT_SHADOW_MASK=0, TRT_SKY_SPANS=0, TRT_SKY_TABLE=0): the knobs
    are read when a context is created.  The caller closes them."""
    made = []
    with pytest.MonkeyPatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        made.append(Renderer(device))
        for knob in OFF:
            mp.setenv(knob, "0")
            made.append(Renderer(device))
            mp.delenv(knob)
    return tuple(made)


def case(w, h, depth, checker):
    sc = S.config_c2(w, h, env_size=ENV)
    fl = (sc.flags & ~T.FLAG_CHECKER) | (T.FLAG_CHECKER if checker else 0)
    return sc, sc.params(max_depth=depth, flags=fl), S.camera_path(sc.ubo, NMAX, SPEED)


def key(w, h, depth, checker):
    return f"{w}x{h}_d{depth}_{'checker' if checker else 'plain'}"


def frames(r, p, ubos):
    """One render_frames call of len(ubos) frames (one launch: at most 64 frames)."""
    import torch

    n = len(ubos)
    out = torch.zeros((n, p.height, p.width, 4), dtype=torch.uint8, device=f"cuda:{r.device}")
    torch.cuda.synchronize(r.device)  # the fill runs on torch's stream, the frames on the context's
    r.render_frames(p, out, n, ubos=ubos, frame_stride=p.height * p.width * 4)
    r.synchronize()
    return out.cpu().numpy()


def single(r, p, ubo):
    r.update_ubo(ubo)
    return r.draw_frame(p)[0]


def digests(a):
    return [hashlib.sha256(np.ascontiguousarray(f).tobytes()).hexdigest() for f in a]


def golden():
    return json.loads(GOLDEN.read_text())
