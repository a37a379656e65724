"""One call site per body in the four sky kernels (sky_trace_kernel_floor / _smask /
sky_trace_kernel / _nospan): single frames and frame pairs reach the same
sky_tile (the primary direction and the sky word once, then sky_frame for one or two frames) and
the same floor_tile (floor_frame in a loop of one or two iterations).  Nothing in the arithmetic
changes, so every frame of a launch of 1, 2, 3, 16, 17 or 33
frames is byte-equal to draw_frame of its own UBO, to the same launch of contexts created under
TRT_FLOOR_CLASS=0, TRT_SHADOW_MASK=0, TRT_SKY_SPANS=0 (the other three sky kernels) and
TRT_SKY_TABLE=0 (trace_kernel), and to the frame the parent commit's build rendered
(tests/golden/one_body_parent_hashes.json: sha256 per frame, recorded on the GPU from that
build).  What would show: a second frame that reads the first frame's FrameRec, camera or span
table, and a light that reads the wrong mask nibble.  draw_frame of the default context runs
sky_tile itself (one frame); what is independent of it is the TRT_SKY_TABLE=0 context and the
parent's hashes.  The walk leaves the spheres after about 21 frames, so the tail of the 33-frame
launch exercises the sky and floor paths, and the sphere-class tiles are covered by the launches
of up to 17 frames.  Run with `pytest -m gpu`."""
from __future__ import annotations

import numpy as np
import pytest

from tests import one_body_common as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs(gpu_renderer):
    made = C.contexts(gpu_renderer.device)
    try:
        yield made
    finally:
        for r in made:
            r.close()


@pytest.fixture(scope="module")
def parent_hashes():
    return C.golden()


@pytest.mark.parametrize("w,h", C.SIZES)
@pytest.mark.parametrize("depth", C.DEPTHS)
@pytest.mark.parametrize("checker", [False, True])
def test_launches(ctxs, parent_hashes, w, h, depth, checker):
    sc, p, ubos = C.case(w, h, depth, checker)
    for r in ctxs:
        r.upload_scene(sc)
    # every frame on its own: a launch of one frame through draw_frame, per context
    ref = np.stack([C.single(ctxs[0], p, u) for u in ubos])
    assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[C.NMAX - 2], ref[C.NMAX - 1])
    for r, name in zip(ctxs[1:], C.NAMES[1:]):
        for k in (0, 1, 16, C.NMAX - 1):
            assert np.array_equal(ref[k], C.single(r, p, ubos[k])), f"draw_frame {k} differs under {name}"
    assert C.digests(ref) == parent_hashes[C.key(w, h, depth, checker)], "differs from the parent commit's frames"
    for n in C.COUNTS:
        for r, name in zip(ctxs, C.NAMES):
            a = C.frames(r, p, ubos[:n])
            bad = [k for k in range(n) if not np.array_equal(a[k], ref[k])]
            assert not bad, f"{n} frames, {name}: frames {bad} differ from draw_frame"
