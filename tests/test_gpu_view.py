"""The view basis on the GPU (abi.h trt_view; trt_kernel.hip primary_dir): a camera that turns.

The chain every test rests on: kernel(view) equals kernel(rays_in = trt_view_rays(view)) bit for
bit, and oracle(rays_in = trt_view_rays(view)) matches kernel(view) under the project's bar with
the geometry counters equal; tests/test_view_host.py closes it on the CPU (trt_view_rays against
numpy float32, the oracle's identity replay).  Every oriented frame is also asserted to differ from
the unrotated one, so a view that is silently ignored fails.  Run with `pytest -m gpu`."""
from __future__ import annotations

import contextlib
import copy

import numpy as np
import pytest

from oracle import oracle as orc
from tests.helpers import assert_float_close, assert_rgba8_close
from vkcomputeshader_tinyraytracer_amd import Renderer, TrtError, scene as S, types as T
from vkcomputeshader_tinyraytracer_amd.multi import MultiRenderer

pytestmark = pytest.mark.gpu

ENV = (64, 32)
V1 = S.view_ypr(20, -10, 5)
V2 = S.view_ypr(-35, -20, 0)
V3 = S.view_ypr(180, 0, 0)  # all sky on C2
SKEW = np.zeros((), T.VIEW)  # finite, neither unit nor orthogonal
SKEW["right"], SKEW["up"], SKEW["back"] = (1.2, 0.1, 0.0), (0.3, 0.9, -0.2), (0.1, -0.2, 1.5)
VIEWS = {"V1": V1, "V2": V2, "SKEW": SKEW}
DEFER_AUTO, DEFER_OFF, DEFER_ON = 0, 1, 2


@contextlib.contextmanager
def viewed(r, view):
    r.set_view(view)
    try:
        yield r
    finally:
        r.set_view(None)


def _counts(st):
    return {k: st[k] for k in T.Stats.EXACT}


def _differs(a8, b8) -> float:
    return float((a8 != b8).any(axis=-1).mean())


def _oracle(sc, p, view):
    """The oracle's frame of `view`: its own primary rays replaced by the host twin's."""
    rays = S.view_rays(p, view)
    q = T.Params.from_buffer_copy(p)
    q.rays_in = rays.ctypes.data
    return orc.render(sc, q, want32=True)


def _check_oracle(r, sc, p, view, plain8):
    """kernel(view): counting launch against the oracle (bar + exact counters), the plain launch
    equal to the counting one, and different from the unrotated frame."""
    with viewed(r, view):
        c8, c32, cst = r.draw_frame(p, count=True, want32=True)
        g8, g32, _ = r.draw_frame(p, want32=True)
    o8, o32, ost = _oracle(sc, p, view)
    assert_rgba8_close(c8, o8)
    assert_float_close(c32, o32)
    assert _counts(cst) == _counts(ost), (cst, ost)
    assert np.array_equal(g8, c8) and np.array_equal(g32, c32)
    assert _differs(g8, plain8) > 0.5
    return g8, g32


def _frames(r, p, ubos, views, batch=0, in_flight=0):
    import torch

    n = len(ubos)
    out = torch.zeros((n, p.height, p.width, 4), dtype=torch.uint8, device=f"cuda:{r.device}")
    torch.cuda.synchronize(r.device)  # the fill runs on torch's stream, the frames on the context's
    r.set_frame_batch(batch)
    r.set_frames_in_flight(in_flight)
    try:
        r.render_frames(p, out, n, ubos=ubos, frame_stride=p.height * p.width * 4, views=views)
        r.synchronize()
    finally:
        r.set_frame_batch(0)
        r.set_frames_in_flight(0)
    return out.cpu().numpy()


def _singles(r, p, ubos, views):
    out = []
    for u, v in zip(ubos, views):
        r.update_ubo(u)
        with viewed(r, v):
            out.append(r.draw_frame(p)[0])
    return out


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("size", [(256, 192), (101, 67)])
@pytest.mark.parametrize("name", list(VIEWS))
def test_c2_view_matches_oracle_and_replay(gpu_renderer, name, size, quirk):
    r = gpu_renderer
    sc = S.config_c2(*size, env_size=ENV)
    if not quirk:
        sc.flags &= ~T.FLAG_ROW_QUIRK
    p = sc.params()
    r.upload_scene(sc)
    plain8 = r.draw_frame(p)[0]
    g8, g32 = _check_oracle(r, sc, p, VIEWS[name], plain8)
    # the host twin replayed through binding 1, no view set: the same frame, both outputs
    y8, y32, _ = r.draw_frame(p, rays_in=S.view_rays(p, VIEWS[name]), want32=True)
    assert np.array_equal(y8, g8) and np.array_equal(y32, g32)


def test_c2_oracle_counts_keep_every_kind_of_ray_in_frame():
    """What the issue measured with the oracle: V1 and V2 keep spheres, floor and sky in frame."""
    sc = S.config_c2(96, 64, env_size=ENV)
    for v in (V1, V2, S.VIEW_IDENTITY):
        st = _oracle(sc, sc.params(), v)[2]
        assert st["misses"] > 3800 and st["secondary_rays"] > 1700 and st["shadow_rays"] > 10000, st


# 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 5, 8, 20])
def test_c2_depths(gpu_renderer, depth):
    """Every stack instantiation of the plain kernel (CAP 0, 4, 7, 19; CAP 3 is case 1)."""
    r = gpu_renderer
    sc = S.config_c2(128, 96, env_size=ENV)
    p = sc.params(max_depth=depth)
    r.upload_scene(sc)
    _check_oracle(r, sc, p, V1, r.draw_frame(p)[0])


# 3 ---------------------------------------------------------------------------------------------
def test_identity_is_todays_path(gpu_renderer):
    r = gpu_renderer
    sc = S.config_c2(264, 200, env_size=ENV)
    p = sc.params()
    r.upload_scene(sc)
    want8, want32, _ = r.draw_frame(p, want32=True)
    for v in (S.VIEW_IDENTITY, None, S.view_ypr(0, 0, 0), S.view_look((0, 0, -1))):
        with viewed(r, V1):
            pass  # a view was in force before
        with viewed(r, v):
            g8, g32, _ = r.draw_frame(p, want32=True)
        assert np.array_equal(g8, want8) and np.array_equal(g32, want32)
    # a 6-frame walk, where the sky table, the spans and the floor class are live
    ubos = S.camera_path(sc.ubo, 6, 0.5)
    want = _frames(r, p, ubos, None)
    ident = np.repeat(S.VIEW_IDENTITY[None], 6)
    assert np.array_equal(_frames(r, p, ubos, ident), want)
    with viewed(r, S.VIEW_IDENTITY):
        assert np.array_equal(_frames(r, p, ubos, None), want)
    singles = _singles(r, p, ubos, [None] * 6)
    for k in range(6):
        assert np.array_equal(want[k], singles[k]), k
    r.update_ubo(sc.ubo)


# 4 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [0, 1, 2])
def test_multi_frame_launches(gpu_renderer, batch):
    """7 frames, 7 views, 7 camera positions in one call: each frame reads its own basis (batch
    2: frame pairs), byte-equal to its single frame."""
    r = gpu_renderer
    sc = S.config_c2(264, 200, env_size=ENV)
    p = sc.params()
    r.upload_scene(sc)
    ubos, views = S.camera_orbit(sc.ubo, 7, speed=0.5, yaw_step=6.0, pitch_step=-2.0, yaw0=-15.0, pitch0=-4.0)
    assert len({v.tobytes() for v in views}) == 7
    got = _frames(r, p, ubos, views, batch=batch)
    want = _singles(r, p, ubos, views)
    plain = _singles(r, p, ubos, [None] * 7)
    for k in range(7):
        assert np.array_equal(got[k], want[k]), k
        assert _differs(got[k], plain[k]) > 0.5, k
    # the context's view serves frames without one of their own
    with viewed(r, views[3]):
        ctx = _frames(r, p, ubos, None, batch=batch)
    same = _singles(r, p, ubos, [views[3]] * 7)
    for k in range(7):
        assert np.array_equal(ctx[k], same[k]), k
    r.update_ubo(sc.ubo)


def test_launch_clamp_and_mixed_frames(gpu_renderer):
    r = gpu_renderer
    sc = S.config_c2(64, 48, env_size=ENV)
    p = sc.params()
    r.upload_scene(sc)
    n = T.MAX_VIEW_FRAMES + 3  # one call, more frames than an oriented launch holds
    ubos, views = S.camera_orbit(sc.ubo, n, speed=0.1, yaw_step=2.0, pitch_step=-0.5, yaw0=3.0)
    got = _frames(r, p, ubos, views)
    want = _singles(r, p, ubos, views)
    for k in range(n):
        assert np.array_equal(got[k], want[k]), k
    # frames of the reference camera among oriented ones, in one launch and across the clamp
    mixed = views.copy()
    for k in (0, 1, 4, 9, 20, n - 1):
        mixed[k] = S.VIEW_IDENTITY
    got = _frames(r, p, ubos, mixed)
    want = _singles(r, p, ubos, mixed)
    for k in range(n):
        assert np.array_equal(got[k], want[k]), k
    r.update_ubo(sc.ubo)


# 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["C3", "shipped"])
def test_meshes(gpu_renderer, golden_meshes, which):
    r = gpu_renderer
    if which == "C3":
        sc, lo, hi = S.config_c3(160, 96, env_size=ENV, level=2), 1815, 2553
    else:
        sc, lo, hi = S.config_reference_default(golden_meshes, env_size=ENV, width=128, height=96), 8753, 9664
    p = sc.params()
    r.upload_scene(sc)
    plain8 = r.draw_frame(p)[0]
    with viewed(r, V1):
        c8, c32, cst = r.draw_frame(p, count=True, want32=True)
        g8, g32, _ = r.draw_frame(p, want32=True)
        w = sc.params()
        w.flags |= T.FLAG_BATCH_WALK
        w8, w32, _ = r.draw_frame(w, want32=True)
    o8, o32, ost = _oracle(sc, p, V1)
    assert lo <= ost["tri_nearest"] <= hi, ost  # the meshes are in frame
    assert_rgba8_close(c8, o8)
    assert_float_close(c32, o32)
    assert _counts(cst) == _counts(ost), (cst, ost)
    assert_rgba8_close(g8, o8)  # the default path (the shipped scene: a deferred frame)
    assert np.array_equal(w8, c8) and np.array_equal(w32, c32)
    assert _differs(g8, plain8) > 0.5


# 6 ---------------------------------------------------------------------------------------------
def _defer_frame(r, p, defer, split=1):
    r.set_deferred_shadows(defer)
    r.set_subtree_split(split)
    try:
        g8, g32, _ = r.draw_frame(p, want32=True)
        return g8, g32
    finally:
        r.set_deferred_shadows(DEFER_AUTO)
        r.set_subtree_split(0)


def test_deferred_and_split(gpu_renderer, golden_meshes, monkeypatch):
    r = gpu_renderer
    sc = S.config_reference_default(golden_meshes, env_size=ENV, width=128, height=96)
    p = sc.params()
    r.upload_scene(sc)
    plain8 = _defer_frame(r, p, DEFER_OFF)[0]
    with viewed(r, V2):
        u8, u32 = _defer_frame(r, p, DEFER_OFF)
        d8, d32 = _defer_frame(r, p, DEFER_ON)
        assert r.defer_stats(0)["fallback_pixels"] == 0
        s8, s32 = _defer_frame(r, p, DEFER_ON, split=3)
        monkeypatch.setenv("TRT_DEFER_EVCAP", "8")
        f8, f32 = _defer_frame(r, p, DEFER_ON)
        nfb = r.defer_stats(0)["fallback_pixels"]
        monkeypatch.delenv("TRT_DEFER_EVCAP")
    assert _differs(u8, plain8) > 0.5
    assert np.array_equal(d8, u8) and np.array_equal(d32, u32)
    assert np.array_equal(s8, u8) and np.array_equal(s32, u32)
    assert nfb > 0  # defer_fallback traced pixels, in the view
    assert np.array_equal(f8, u8) and np.array_equal(f32, u32)


@pytest.mark.parametrize("in_flight", [0, 2])
def test_deferred_frame_groups(gpu_renderer, golden_meshes, in_flight):
    r = gpu_renderer
    sc = S.config_reference_default(golden_meshes, env_size=ENV, width=128, height=96)
    p = sc.params()
    r.upload_scene(sc)
    ubos, views = S.camera_orbit(sc.ubo, 5, speed=0.05, yaw_step=5.0, pitch_step=-2.0, yaw0=-30.0, pitch0=-12.0)
    r.set_deferred_shadows(DEFER_ON)
    try:
        got = _frames(r, p, ubos, views, in_flight=in_flight)
        want = _singles(r, p, ubos, views)
    finally:
        r.set_deferred_shadows(DEFER_AUTO)
        r.update_ubo(sc.ubo)
    for k in range(5):
        assert np.array_equal(got[k], want[k]), k


# 7 ---------------------------------------------------------------------------------------------
def test_bands(gpu_renderer):
    torch = pytest.importorskip("torch")
    r = gpu_renderer
    sc = S.config_c2(96, 64, env_size=ENV)
    r.upload_scene(sc)
    plain8 = r.draw_frame(sc.params())[0]
    with viewed(r, V1):
        full, full32, _ = r.draw_frame(sc.params(), want32=True)
        out8 = torch.zeros((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda")
        out32 = torch.zeros((sc.height, sc.width, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # the fill ran on the default stream: order it before our streams
        for idx in range(3):
            p = sc.params(band_rows=8, band_count=3, band_index=idx)
            band = r.draw_frame(p)[0]
            assert np.array_equal(band, full[T.output_rows(sc.height, 8, 3, idx)]), idx
            p.flags |= T.FLAG_BAND_IN_PLACE
            r.draw_frame(p, out8=out8, out32=out32)
        torch.cuda.synchronize()
    assert _differs(full, plain8) > 0.5
    assert np.array_equal(out8.cpu().numpy(), full)
    assert np.array_equal(out32.cpu().numpy(), full32)


# 8 ---------------------------------------------------------------------------------------------
def test_spp(gpu_renderer):
    """spp 16 on a small mesh scene: the lane-per-sample path (the default) and the per-pixel
    sample loop (a context created under TRT_SPP_LANES=0) turn every jittered sample alike.  No
    oracle comparison: rays_in holds one ray per pixel, so the jittered, rotated samples cannot be
    replayed through it."""
    sc = S.config_c4(96, 64, env_size=ENV, n_objects=4, level=1, spp=16)
    p = sc.params()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("TRT_SPP_LANES", "0")
        loop = Renderer(gpu_renderer.device)
    try:
        loop.upload_scene(sc)
        gpu_renderer.upload_scene(sc)
        plain8 = gpu_renderer.draw_frame(p)[0]
        with viewed(gpu_renderer, V1), viewed(loop, V1):
            a8, a32, _ = gpu_renderer.draw_frame(p, want32=True)
            b8, b32, _ = loop.draw_frame(p, want32=True)
    finally:
        loop.close()
    assert np.array_equal(a8, b8) and np.array_equal(a32, b32)
    assert _differs(a8, plain8) > 0.5


# 9 ---------------------------------------------------------------------------------------------
def test_multi_gpu_on_one_gpu(gpu_renderer):
    torch = pytest.importorskip("torch")
    r = gpu_renderer
    sc = S.config_c2(236, 90, env_size=ENV)
    p = sc.params()
    r.upload_scene(sc)
    plain8 = r.draw_frame(p)[0]
    ubos = S.camera_path(sc.ubo, 4, 0.3)
    want = _singles(r, p, ubos, [V1] * 4)
    r.update_ubo(sc.ubo)
    with viewed(r, V1):
        whole = r.draw_frame(p)[0]
    m = MultiRenderer([0])
    try:
        m.set_band_groups(3)
        m.set_self_gather(True)
        m.upload_scene(sc)
        m.set_view(V1)
        one = np.zeros_like(whole)
        m.draw_frame(p, band_rows=8, root=0, outs=[one])
        out = torch.zeros((4, p.height, p.width, 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        m.render_frames(p, 4, band_rows=8, root=0, frames_per_gather=3, outs=[out],
                        frame_stride=p.height * p.width * 4, ubos=ubos)
        m.synchronize()
        got = out.cpu().numpy()
        m.set_view(None)
        back = np.zeros_like(whole)
        m.update_ubo(sc.ubo)
        m.draw_frame(p, band_rows=8, root=0, outs=[back])
    finally:
        m.close()
    assert np.array_equal(one, whole) and _differs(whole, plain8) > 0.5
    for k in range(4):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(back, plain8)


# 10 --------------------------------------------------------------------------------------------
def test_errors_and_rays_in_wins(gpu_renderer):
    r = gpu_renderer
    sc = S.config_c2(96, 64, env_size=ENV)
    p = sc.params()
    r.upload_scene(sc)
    plain8 = r.draw_frame(p)[0]
    with viewed(r, V1):
        v1 = r.draw_frame(p)[0]
        for bad_value in (float("nan"), float("inf")):
            bad = copy.deepcopy(V2)
            bad["up"][1] = bad_value
            with pytest.raises(TrtError):
                r.set_view(bad)
            assert np.array_equal(r.draw_frame(p)[0], v1)  # the previous view stays in force
        # rays_in wins over the view: the directions are the caller's
        y8 = r.draw_frame(p, rays_in=S.view_rays(p, V2))[0]
        i8 = r.draw_frame(p, rays_in=S.view_rays(p, None))[0]
    with viewed(r, V2):
        v2 = r.draw_frame(p)[0]
    assert np.array_equal(y8, v2) and np.array_equal(i8, plain8)
    assert _differs(v1, plain8) > 0.5 and _differs(v2, v1) > 0.5
    import torch

    out = torch.zeros((2, p.height, p.width, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bad = np.stack([V1, V2])
    bad[1]["back"][2] = float("nan")
    with pytest.raises(TrtError):
        r.render_frames(p, out, 2, frame_stride=p.height * p.width * 4, views=bad)
    r.synchronize()
