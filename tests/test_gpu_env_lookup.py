"""The envmap lookup on the GPU (env_fetch / env_blend in trt_kernel.hip, the pair rows built by
envp_kernel) as its own operation, over tests/env_lookup_common.py's shapes and rays: directed rays
through ray_query_kernel against the float64 reference and the oracle; the three fetch paths (pair
rows, 8-byte pairs with TRT_ENV_PAIRROWS=0, scalar at W == 1) bit for bit; frames of an
envmap-only scene and of C2 through the frame kernels with the sky table on and off; and the
context's state across uploads of maps of other sizes and row strides, a JPEG upload included.
Run with `pytest -m gpu`."""
from __future__ import annotations

import copy
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as orc
from tests import env_lookup_common as E
from tests.helpers import assert_float_close, assert_rgba8_close
from vkcomputeshader_tinyraytracer_amd import Renderer, scene as S, types as T

pytestmark = pytest.mark.gpu

SHAPES = pytest.mark.parametrize("shape", E.ENV_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
FW, FH = 72, 40  # nine 8x8 tile columns, five tile rows: one wave and a partial one per row of tiles
JPEG = Path(__file__).resolve().parent / "golden" / "jpeg" / "b444_q90_37x23.jpg"
VIEWS = {"reference": None, "seam": (-1.0, 0.0, 0.0), "north": (0.0, 1.0, -1e-3), "south": (0.0, -1.0, -1e-3)}


@pytest.fixture
def ctx(gpu_renderer):
    r = gpu_renderer
    yield r
    r.set_view(None)
    r.set_stream(None)


@pytest.fixture(scope="module")
def table_off(gpu_renderer):
    """A context without the sky table: the knob is read when a context is created."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("TRT_SKY_TABLE", "0")
        r = Renderer(gpu_renderer.device)
    yield r
    r.close()


@pytest.fixture(scope="module")
def lit_off(gpu_renderer):
    """A context whose floor-class launches run sky_trace_kernel_floor, not its lit variant."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("TRT_FLOOR_LIT", "0")
        r = Renderer(gpu_renderer.device)
    yield r
    r.close()


def _upload(r, sc, view=None):
    r.upload_scene(sc)  # always afresh: ensure_envp reads TRT_ENV_PAIRROWS after each upload
    r.update_ubo(sc.ubo)
    r.set_view(view)


def _directed(r, sc, rays):
    g8, g32, _, st = r.trace_rays(rays, sc.params(), want32=True, count=True)
    n = len(rays)
    assert st["misses"] == n and st["primary_rays"] == n and st["secondary_rays"] == 0
    return g8, g32


def _check_directed(g8, g32, c, rays, label, seam=None):
    """Every ray against ref64 under the bar and against the oracle's bytes within 1."""
    d = np.abs(g32[:, :3].astype(np.float64) - c["r64"]["gamma"])
    i = int(d.max(axis=1).argmax())
    print(f"envlookup {label}: {len(rays)} rays, gpu vs ref64 {d.max():.3g} (bar {c['tol']:.3g}; oracle vs ref64 "
          f"linear {c['E_lin']:.3g}, gamma'd {c['E_gamma']:.3g}), worst ray {i} dir {rays['dir'][i].tolist()}")
    assert np.isfinite(g32).all()
    assert d.max() <= c["tol"], (label, float(d.max()), c["tol"], i, rays["dir"][i])
    assert (g32[:, 3] == 1.0).all() and (g8[:, 3] == 255).all()
    d8 = np.abs(g8.astype(np.int16) - c["ref8"].astype(np.int16))
    assert d8.max() <= 1, (label, int(d8.max()), rays["dir"][int(d8.max(axis=1).argmax())])
    if seam is not None:
        for idx in seam:
            assert g8[idx].tobytes() == c["ref8"][idx].tobytes()


# ---- 3a: directed rays --------------------------------------------------------------------------


@SHAPES
def test_directed_rays(ctx, shape):
    c = E.shape_case(shape)
    sc = E.env_scene(c["env"])
    _upload(ctx, sc)
    g8, g32 = _directed(ctx, sc, c["rays"])
    _check_directed(g8, g32, c, c["rays"], f"{shape[0]}x{shape[1]}", E.seam_rays(*shape))


# ---- 3b: the fetch paths ------------------------------------------------------------------------


def _both_paths(r, sc, run, view=None):
    """run(r) with the pair rows, then without them (the pair path, or the scalar one at W == 1);
    leaves the context with the scene uploaded and its pair rows back."""
    _upload(r, sc, view)
    a = run(r)
    try:
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("TRT_ENV_PAIRROWS", "0")
            _upload(r, sc, view)
            b = run(r)
    finally:
        _upload(r, sc, view)
    return a, b


@SHAPES
def test_fetch_paths_agree(ctx, shape):
    c = E.shape_case(shape)
    sc = E.env_scene(c["env"])
    (a8, a32), (b8, b32) = _both_paths(ctx, sc, lambda r: _directed(r, sc, c["rays"]))
    assert np.array_equal(a8, b8) and np.array_equal(a32, b32)
    g8, g32 = _directed(ctx, sc, c["rays"])  # and the pair rows are back
    assert np.array_equal(a8, g8) and np.array_equal(a32, g32)


# ---- 3c: frames ---------------------------------------------------------------------------------


def _oracle_frame(sc, p, view):
    if view is None:
        return orc.render(sc, p, want32=True)
    rays = S.view_rays(p, view)
    q = T.Params.from_buffer_copy(p)
    q.rays_in = rays.ctypes.data
    return orc.render(sc, q, want32=True)


@pytest.mark.parametrize("name", list(VIEWS))
@pytest.mark.parametrize("shape", [(67, 33), (3, 2), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sky_frames(ctx, table_off, shape, name):
    """An envmap-only frame: the reference camera, the seam down the middle of the frame, a pole
    in frame.  Each is drawn plain (RGBA8 only) and with rayOut, on a context with the sky table and
    on one without, with the pair rows and without them; all equal the oracle under the suite's
    bars and each other byte for byte.  Only the plain reference-camera frame takes the table
    (sky_kernel's lookup, then the table's words): a frame that writes rayOut or is drawn under a
    view stands aside from it by design (attach_sky), so for the three views and for every rayOut
    frame the two contexts run the same per-ray path and the comparison is of fetch paths only."""
    view = None if VIEWS[name] is None else S.view_look(VIEWS[name])
    sc = E.env_scene(E.shape_case(shape)["env"], FW, FH)
    p = sc.params()
    o8, o32, _ = _oracle_frame(sc, p, view)

    def run(r):
        plain8 = r.draw_frame(p)[0]  # first after the upload: builds the table where one is taken
        g8, g32, _ = r.draw_frame(p, want32=True)
        return plain8, g8, g32, r.draw_frame(p)[0]  # and the table serves the next plain frame

    frames = []
    try:
        for r in (ctx, table_off):
            frames += _both_paths(r, sc, run, view)
    finally:
        table_off.set_view(None)
    assert_rgba8_close(frames[0][0], o8)
    assert_rgba8_close(frames[0][1], o8)
    err = assert_float_close(frames[0][2], o32)
    print(f"envlookup frame {shape[0]}x{shape[1]} {name}: rayOut max |d| {err:.3g}")
    for plain8, g8, g32, again8 in frames:
        assert plain8.tobytes() == frames[0][0].tobytes() and again8.tobytes() == frames[0][0].tobytes()
        assert g8.tobytes() == frames[0][0].tobytes() and g32.tobytes() == frames[0][2].tobytes()
    if shape != (1, 1):
        assert len(np.unique(o8.reshape(-1, 4), axis=0)) > 8  # the frame shows the map, not one colour


def _c2_scene():
    return S.Scene("C2", S.make_ubo(), env=E.shape_case((67, 33))["env"], width=FW, height=FH, max_depth=4,
                   flags=T.FLAG_SPHERES | T.FLAG_FLOOR | T.FLAG_ENVMAP | T.FLAG_ROW_QUIRK)


def test_c2_frame_on_random_bytes(ctx, table_off):
    """C2 (spheres and floor) over the random-byte 67x33 map, one frame per launch.  The plain
    frame (RGBA8 only) is the one the sky table, the spans and the occluder masks serve
    (sky_trace_kernel_smask), so its secondary misses take the lookup from that kernel; a launch of
    one frame never takes the floor class (attach_floor_class: test_c2_frame_loop_on_random_bytes
    below).  The rayOut frame and the counting frame stand aside from all of them (attach_sky,
    fill_spans) and give the floats and the counters.  On a context with the table and on one
    without, with the pair rows and without them."""
    sc = _c2_scene()
    p = sc.params()
    o8, o32, ost = orc.render(sc, p, want32=True)

    def run(r):
        plain8 = r.draw_frame(p)[0]
        g8, g32, _ = r.draw_frame(p, want32=True)
        c8, c32, cst = r.draw_frame(p, want32=True, count=True)
        return plain8, g8, g32, c8, c32, cst

    runs = _both_paths(ctx, sc, run) + _both_paths(table_off, sc, run)
    a = runs[0]
    for k in (0, 1, 3):
        assert_rgba8_close(a[k], o8)
    assert_float_close(a[2], o32)
    assert_float_close(a[4], o32)
    assert a[1].tobytes() == a[0].tobytes() and a[3].tobytes() == a[0].tobytes()
    assert ost["secondary_rays"] > 0 and ost["misses"] > 0
    for b in runs:
        assert {k: b[5][k] for k in T.Stats.EXACT} == {k: ost[k] for k in T.Stats.EXACT}
        for x, y in zip(a[:5], b[:5]):
            assert x.tobytes() == y.tobytes()


def _loop(r, p, ubos):
    """render_frames of these UBOs as one launch of plain frames: (n, H, W, 4) uint8."""
    import torch

    n = len(ubos)
    out = torch.zeros((n, p.height, p.width, 4), dtype=torch.uint8, device=f"cuda:{r.device}")
    torch.cuda.synchronize(r.device)  # the fill runs on torch's stream, the frames on the context's
    r.render_frames(p, out, n, ubos=ubos, frame_stride=p.height * p.width * 4)
    r.synchronize()
    return out.cpu().numpy()


def test_c2_frame_loop_on_random_bytes(ctx, lit_off, table_off):
    """The floor class runs only in launches of two frames or more (attach_floor_class), the way
    frame loops and the benchmark launch: a three-frame camera walk of C2 over the random-byte
    67x33 map through render_frames (a frame pair and an odd last frame), on the default context
    (sky_trace_kernel_floor_lit: the reference's lights are above the floor), on one created with
    TRT_FLOOR_LIT=0 (sky_trace_kernel_floor) and on one without the table (trace_kernel), with the
    pair rows and without them.  Every frame equals the oracle's under the bar, the same frame drawn
    alone (draw_frame, no class) byte for byte, and every other run."""
    from tests.floor_class_common import floor_tiles, intervals

    sc = _c2_scene()
    p = sc.params()
    ubos = S.camera_path(sc.ubo, 3, 0.5)
    iv = intervals(p, ubos)
    assert iv is not None and floor_tiles(*iv) > 0  # the launch has floor-class tiles

    def run(r):
        frames = _loop(r, p, ubos)
        alone = []
        for u in ubos:
            r.update_ubo(u)
            alone.append(r.draw_frame(p)[0])
        r.update_ubo(sc.ubo)
        return frames, np.stack(alone)

    runs = _both_paths(ctx, sc, run) + _both_paths(lit_off, sc, run) + _both_paths(table_off, sc, run)
    first = runs[0][0]
    for k in range(len(ubos)):
        at = copy.copy(sc)
        at.ubo = ubos[k]
        assert_rgba8_close(first[k], orc.render(at, p)[0])
    assert not np.array_equal(first[0], first[2])  # the walk moved what is seen
    for frames, alone in runs:
        assert frames.tobytes() == first.tobytes() and alone.tobytes() == first.tobytes()


# ---- 3d: state across uploads -------------------------------------------------------------------


def test_uploads_in_sequence(gpu_renderer):
    """One context through maps of other sizes and row strides: the pair-row buffer is kept when a
    smaller map follows a larger one, and every upload (a JPEG's too) invalidates the rows and the
    sky table built for the map before it.  The 16x8 frame is drawn plain, so it is the table's
    (same size, flags and camera throughout: only the envmap's generation tells the uploads
    apart), and once more with rayOut, which is traced per ray."""

    def frame(r, sc):
        p = sc.params(width=16, height=8)
        o8, o32, _ = orc.render(sc, p, want32=True)
        plain8 = r.draw_frame(p)[0]
        f8, f32_, _ = r.draw_frame(p, want32=True)
        assert_rgba8_close(plain8, o8)
        assert_float_close(f32_, o32)
        assert plain8.tobytes() == f8.tobytes()
        return plain8

    steps = [((257, 2), E.SEED), ((3, 2), E.SEED), ((67, 33), E.SEED), ((1, 1), E.SEED), ((67, 33), E.SEED + 1)]
    with Renderer(gpu_renderer.device) as r:
        seen = []
        for shape, seed in steps:
            c = E.shape_case(shape, seed)
            sc = E.env_scene(c["env"])
            _upload(r, sc)
            g8, g32 = _directed(r, sc, c["rays"])
            _check_directed(g8, g32, c, c["rays"], f"sequence {shape[0]}x{shape[1]} seed {seed}")
            seen.append(frame(r, sc).tobytes())
        r.upload_envmap_jpeg(JPEG)
        env = r.decode_jpeg(JPEG)
        assert env.shape == (23, 37, 4)
        rays = E.directions(37, 23)
        c = E.measure(env, rays)
        sc = E.env_scene(env)  # what the context now holds: for the params and for the oracle
        g8, g32 = _directed(r, sc, rays)
        _check_directed(g8, g32, c, rays, "sequence jpeg 37x23")
        seen.append(frame(r, sc).tobytes())
        assert len(set(seen)) == len(seen)  # a stale table would repeat a frame
