"""Every launch's dealing of blocks to (tile, frame) by the host's constants and magic divisors
(KArgs::deal, csrc/trt_deal.h).  Only how a workgroup finds its (tile, pair)
changed, so every frame of a launch of 2, 3, 16, 17 or 33 frames must be byte-equal to draw_frame
of its own UBO (a single-frame launch, dealt by xcd_tile alone).  136x104 has 8 chunk columns, an
odd right tile column and an odd bottom tile row, whose leftover tiles are dealt after the whole
chunk groups (the division by ntiles - per); 256x96 has two chunk groups per chunk row.  What
would show: a tile dealt twice or never (a frame keeps zeros or another frame's pixels there), a
pair index that no longer matches its span table or FrameRec, a span word read for the wrong tile
row.  The same launches through MultiRenderer at one rank with 8-row bands.  (The row order of
pair launches that this file's name speaks of did not meet its gate and is not built, so there is
no TRT_DEAL_ROWS=0 context to compare with: DESIGN.md 7.)  Run with `pytest -m gpu`."""
from __future__ import annotations

import numpy as np
import pytest

from tests import one_body_common as C
from vkcomputeshader_tinyraytracer_amd import Renderer, scene as S, types as T
from vkcomputeshader_tinyraytracer_amd.multi import MultiRenderer

pytestmark = pytest.mark.gpu

SIZES = [(136, 104), (256, 96)]
DEPTHS = [4, 5]
COUNTS = [2, 3, 16, 17, 33]
NMAX = max(COUNTS)


def _default(make):
    """A context created with none of the knobs set."""
    with pytest.MonkeyPatch.context() as mp:
        for k in C.KNOBS:
            mp.delenv(k, raising=False)
        return make()


@pytest.fixture(scope="module")
def ctx(gpu_renderer):
    r = _default(lambda: Renderer(gpu_renderer.device))
    try:
        yield r
    finally:
        r.close()


@pytest.fixture(scope="module")
def multi(gpu_renderer):
    m = _default(lambda: MultiRenderer([gpu_renderer.device]))
    try:
        yield m
    finally:
        m.close()


_REF: dict = {}


def _case(gpu_renderer, w, h, depth, checker):
    """(scene, params, UBOs along camera_path, every frame by draw_frame): computed once per case
    and shared by both tests, read only."""
    k = (w, h, depth, checker)
    if k not in _REF:
        sc = S.config_c2(w, h, env_size=C.ENV)
        fl = (sc.flags & ~T.FLAG_CHECKER) | (T.FLAG_CHECKER if checker else 0)
        p, ubos = sc.params(max_depth=depth, flags=fl), S.camera_path(sc.ubo, NMAX, C.SPEED)
        gpu_renderer.upload_scene(sc)
        ref = np.stack([C.single(gpu_renderer, p, u) for u in ubos])
        ref.setflags(write=False)
        assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[NMAX - 2], ref[NMAX - 1])
        _REF[k] = (sc, p, ubos, ref)
    return _REF[k]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("checker", [False, True])
def test_render_frames(gpu_renderer, ctx, w, h, depth, checker):
    sc, p, ubos, ref = _case(gpu_renderer, w, h, depth, checker)
    ctx.upload_scene(sc)
    for n in COUNTS:
        a = C.frames(ctx, p, ubos[:n])
        bad = [k for k in range(n) if not np.array_equal(a[k], ref[k])]
        assert not bad, f"{n} frames: frames {bad} differ from draw_frame"


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("checker", [False, True])
def test_multi_renderer_bands(gpu_renderer, multi, w, h, depth, checker):
    import torch

    sc, p, ubos, ref = _case(gpu_renderer, w, h, depth, checker)
    fb = p.height * p.width * 4
    multi.upload_scene(sc)
    for n in COUNTS:
        out = torch.zeros((n, p.height, p.width, 4), dtype=torch.uint8, device=f"cuda:{gpu_renderer.device}")
        torch.cuda.synchronize(gpu_renderer.device)  # the fill ran on torch's stream
        multi.render_frames(p, n, band_rows=8, root=0, frames_per_gather=n, outs=[out], frame_stride=fb, ubos=ubos[:n])
        multi.synchronize()
        a = out.cpu().numpy()
        bad = [k for k in range(n) if not np.array_equal(a[k], ref[k])]
        assert not bad, f"{n} frames, MultiRenderer: frames {bad} differ from draw_frame"
