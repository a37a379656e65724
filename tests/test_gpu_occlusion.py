"""Occlusion queries on the GPU (abi.h trt_occluded, occlusion_query_kernel): the strict boundary at
a ray's own hit distance, the identity occluded(ray, tmax) == (hit.t < tmax) against the oracle
and against the GPU's own hit records, every mesh path, the adversarial meshes, the wave-coherent
shadow walk entered by ragged waves with bad lanes gone, host rejection, sizes, streams and side
effects.  Every comparison of occlusion bytes is exact.  None of these provokes a fault: a bad
record is inert by contract and a misaligned call is refused on the host."""
from __future__ import annotations

import numpy as np
import pytest

from tests import mesh_cases as M
from tests.occlusion_common import (boundary_segments, expected_occluded, hits_for, hits_without_floor)
from tests.query_common import f32, random_rays
from vkcomputeshader_tinyraytracer_amd import Renderer, TrtError, scene as S, types as T

pytestmark = pytest.mark.gpu

W, H = 71, 41
KS = (f32(0.999), f32(1.0), f32(1.001))
BAD = [0, 63, 64, 129]


@pytest.fixture(scope="module")
def scenes():
    c2 = S.config_c2(W, H, env_size=(64, 32))
    c3 = S.config_c3(W, H, env_size=(64, 32), level=2)  # a 320-triangle glass icosphere
    return {"C2": c2, "C3": c3}


@pytest.fixture
def use(gpu_renderer):
    """Uploads a scene into the session's context and hands it back in its default state."""
    r = gpu_renderer

    def _use(sc):
        if r.scene is not sc:
            r.upload_scene(sc)
        r.update_ubo(sc.ubo)
        r.set_view(None)
        return r

    yield _use
    r.set_view(None)
    r.set_stream(None)
    if r.scene is not None:
        r.update_ubo(r.scene.ubo)


@pytest.fixture(scope="module")
def g2(gpu_renderer):
    """A context created under TRT_BVH_WAVES4=0: mesh scenes take the GEOM 2 kernels (the knob is
    read when a context is created)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("TRT_BVH_WAVES4", "0")
        made = Renderer(gpu_renderer.device)
    try:
        yield made
    finally:
        made.close()


def _no_floor(sc) -> int:
    return int(sc.flags) & ~T.FLAG_FLOOR


# ---- 1: the boundary ----------------------------------------------------------------------------


@pytest.fixture(scope="module")
def boundary(scenes):
    """Per scene: random_rays(2053, 77), their oracle records with and without the floor, the
    boundary segments around the records with the floor, and each segment's ray."""
    out = {}
    for name, sc in scenes.items():
        rays = random_rays(2053, 77)
        on = hits_for(sc, rays, sc.flags)
        kinds = {k: int((on["kind"] == k).sum()) for k in (T.HIT_NONE, T.HIT_FLOOR, T.HIT_SPHERE, T.HIT_TRIANGLE)}
        assert kinds[T.HIT_NONE] and kinds[T.HIT_FLOOR] and kinds[T.HIT_SPHERE] and (name == "C2" or kinds[T.HIT_TRIANGLE]), kinds
        off = hits_without_floor(sc, rays, on)
        segs, idx = boundary_segments(rays, on)
        out[name] = (rays, on, off, segs, idx)
    return out


@pytest.mark.parametrize("floor", [True, False], ids=["floor", "nofloor"])
@pytest.mark.parametrize("name", ["C2", "C3"])
def test_boundary_at_the_hit_distance(use, scenes, boundary, name, floor):
    sc = scenes[name]
    rays, on, off, segs, idx = boundary[name]
    flags = sc.flags if floor else _no_floor(sc)
    want = expected_occluded(sc, segs, flags, (on if floor else off)[idx])
    hit = on["kind"][idx] != T.HIT_NONE
    trip = want[hit].reshape(-1, 3)
    if floor:  # tmax = t is clear (strict), the next float is occluded; a miss is clear
        assert (trip[:, 0] == T.OCC_VISIBLE).all() and (trip[:, 1] == T.OCC_OCCLUDED).all()
    else:      # ... for every hit but the floor's, which dropped out of the reference
        nf = on["kind"][idx][hit].reshape(-1, 3)[:, 0] != T.HIT_FLOOR
        assert (trip[nf, 0] == T.OCC_VISIBLE).all() and (trip[nf, 1] == T.OCC_OCCLUDED).all()
        assert (trip[~nf, 1] == T.OCC_VISIBLE).any()
    assert (want[~hit] == T.OCC_VISIBLE).all()
    r = use(sc)
    got = r.occluded(segs, sc.params(flags=flags))
    assert got.dtype == np.uint8 and got.shape == (len(segs),)
    print(f"{name} floor={floor}: {len(segs)} segments, {int(want.sum())} occluded, {int((got != want).sum())} differ")
    assert got.tobytes() == want.tobytes()


# ---- 2, 3: the identity against the GPU's own records, on every mesh path ------------------------


def aimed_rays() -> np.ndarray:
    """The ray set of tests/test_gpu_query.py's c3_refs: random_rays(1027, 4242) with every second
    ray starting near the mesh and aimed at it."""
    rays = random_rays(1027, 4242)
    rng = np.random.default_rng(99)
    aim = np.arange(0, len(rays), 2)
    rays["org"][aim] = (np.array((2.5, -2.0, -10.0)) + rng.uniform(-4, 4, size=(len(aim), 3))).astype(f32)
    rays["dir"][aim] = (np.array((2.5, -2.0, -10.0)) + rng.uniform(-1.2, 1.2, size=(len(aim), 3)) - rays["org"][aim]).astype(f32)
    return rays


def scaled_segments(rays, t):
    """Three segments per ray, tmax = k t for k in KS in float32, held inside the valid range (a
    miss's 1.001 x 1e10 would not be a valid segment)."""
    t = np.asarray(t, f32)
    tm = np.minimum(np.stack([k * t for k in KS], 1).astype(f32), T.QSEG_MAX_T)
    idx = np.repeat(np.arange(len(rays)), len(KS))
    return S.segments_from_rays(rays[idx], tm.reshape(-1)), idx


@pytest.fixture(scope="module")
def aimed(scenes):
    sc = scenes["C3"]
    rays = aimed_rays()
    want = hits_for(sc, rays, sc.flags)
    assert int((want["kind"] == T.HIT_TRIANGLE).sum()) > 100
    return rays, want


def test_identity_against_the_gpus_own_records(use, scenes, aimed):
    sc = scenes["C3"]
    rays, _ = aimed
    r = use(sc)
    p = sc.params()
    _, _, hits, _ = r.trace_rays(rays, p, want8=False, want_hits=True)
    segs, idx = scaled_segments(rays, hits["t"])
    got = r.occluded(segs, p)
    want = (hits["t"][idx] < segs["tmax"]).astype(np.uint8)
    assert want.any() and not want.all()
    assert got.tobytes() == want.tobytes()


def test_every_mesh_path(use, scenes, aimed, g2):
    """The default quantized BVH (GEOM 3), the reference-order batch walk (TRT_FLAG_BATCH_WALK, GEOM
    1) and the unquantized BVH of a TRT_BVH_WAVES4=0 context (GEOM 2): byte-equal to the oracle's
    reference and to each other."""
    sc = scenes["C3"]
    rays, hits = aimed
    segs, idx = scaled_segments(rays, hits["t"])
    want = expected_occluded(sc, segs, sc.flags, hits[idx])
    assert want.any() and not want.all()
    r = use(sc)
    a = r.occluded(segs, sc.params())
    b = r.occluded(segs, sc.params(flags=sc.flags | T.FLAG_BATCH_WALK))
    g2.upload_scene(sc)
    c = g2.occluded(segs, sc.params())
    for path, got in (("GEOM 3", a), ("GEOM 1", b), ("GEOM 2", c)):
        assert got.tobytes() == want.tobytes(), path


# ---- 4: adversarial meshes ------------------------------------------------------------------------


def _query_rays(sc, seed):
    """The ray set tests/test_gpu_mesh_cases.py traces for a case's queries: 1027 free rays; every
    second one aims at a point drawn inside a triangle drawn from the mesh (of those within 100
    units that have an area) and starts within 4 units of that point."""
    rays = random_rays(1027, seed)
    rng = np.random.default_rng(seed + 1)
    aim = np.arange(0, len(rays), 2)
    v = np.stack([sc.tris[k][:, :3] for k in ("v0", "v1", "v2")], 1).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        area = np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
    big = np.flatnonzero((area > 1e-3) & (np.abs(v).max(axis=(1, 2)) < 100.0))
    pick = v[rng.choice(big, len(aim))]
    w = rng.dirichlet((1.0, 1.0, 1.0), len(aim))
    target = np.einsum("nk,nkc->nc", w, pick)
    org = target + rng.uniform(-4, 4, size=target.shape)
    rays["org"][aim] = org.astype(f32)
    rays["dir"][aim] = (target - rays["org"][aim].astype(np.float64)).astype(f32)
    return rays


@pytest.fixture(scope="module")
def adversarial():
    out = {}
    for i, name in enumerate(M.QUERY_CASES):
        sc = M.CASES[name].scene
        rays = _query_rays(sc, 7000 + i)
        hits = hits_for(sc, rays, sc.flags)
        assert int((hits["kind"] == T.HIT_TRIANGLE).sum()) > 100
        segs, idx = boundary_segments(rays, hits)
        want = expected_occluded(sc, segs, sc.flags, hits[idx])
        assert (want == T.OCC_OCCLUDED).any() and (want == T.OCC_VISIBLE).any()
        out[name] = (segs, want)
    return out


@pytest.mark.parametrize("name", M.QUERY_CASES)
def test_adversarial_meshes(use, g2, adversarial, name):
    sc = M.CASES[name].scene
    segs, want = adversarial[name]
    r = use(sc)
    a = r.occluded(segs, sc.params())
    b = r.occluded(segs, sc.params(flags=sc.flags | T.FLAG_BATCH_WALK))
    g2.upload_scene(sc)
    c = g2.occluded(segs, sc.params())
    for path, got in (("default", a), ("batch walk", b), ("TRT_BVH_WAVES4=0", c)):
        print(f"{name} {path}: {int((got != want).sum())} of {len(want)} differ")
        assert got.tobytes() == want.tobytes(), path


# ---- 5, 6: the coherent-wave path with ragged waves; host rejection -------------------------------

CLUSTER = (2.2, -3.9, -9.6)  # just above the floor, under the icosphere (centre (2.5, -2, -10), radius 1.5)


@pytest.fixture(scope="module")
def cluster(scenes):
    """130 segments from origins within 0.05 of CLUSTER (inside TRT_SHADOW_WAVE_EXT = 0.1 of each
    other's first, so a wave of them takes the wave-cooperative walk) to the scene's three lights,
    the oracle's verdicts, and the same array with records 0, 63, 64 and 129 made bad."""
    sc = scenes["C3"]
    rng = np.random.default_rng(31)
    org = (np.asarray(CLUSTER) + rng.uniform(-0.045, 0.045, size=(130, 3))).astype(f32)
    assert np.abs(org.astype(np.float64) - np.asarray(CLUSTER)).max() <= 0.05
    lights = np.array([sc.ubo[f"light{i}"][:3] for i in range(3)], f32)
    good = S.segments_between(org, lights[np.arange(130) % 3])
    want = expected_occluded(sc, good, sc.flags)
    assert (want == T.OCC_OCCLUDED).any() and (want == T.OCC_VISIBLE).any(), "move the cluster"
    bad = good.copy()
    bad["dir"][0] = (np.nan, 0.0, -1.0)
    bad["dir"][63] = 0.0
    bad["org"][64, 1] = np.inf
    bad["tmax"][129] = np.nan
    return good, want, bad


def test_coherent_wave_with_ragged_waves_and_bad_lanes(use, scenes, cluster):
    torch = pytest.importorskip("torch")
    sc = scenes["C3"]
    good, want, bad = cluster
    r = use(sc)
    p = sc.params()
    host = r.occluded(good, p)
    assert host.tobytes() == want.tobytes()
    dev = torch.from_numpy(bad.view(np.uint8).reshape(130, 32)).to(f"cuda:{r.device}")
    torch.cuda.synchronize(r.device)
    got = r.occluded(dev, p)
    r.synchronize()
    assert got.dtype == torch.uint8 and got.shape == (130,) and got.is_cuda
    got = got.cpu().numpy()
    rest = np.setdiff1d(np.arange(130), BAD)
    assert (got[BAD] == T.OCC_BAD_SEG).all()
    assert got[rest].tobytes() == host[rest].tobytes() == want[rest].tobytes()
    # the good array from the device: the same bytes as through host pointers
    gdev = torch.from_numpy(good.view(np.uint8).reshape(130, 32)).to(f"cuda:{r.device}")
    torch.cuda.synchronize(r.device)
    again = r.occluded(gdev, p)
    r.synchronize()
    assert again.cpu().numpy().tobytes() == host.tobytes()


def test_host_rejection(use, scenes, cluster):
    sc = scenes["C3"]
    _, _, bad = cluster
    r = use(sc)
    out = np.full(130, 0xA5, np.uint8)
    with pytest.raises(TrtError, match=r"segment 0 ") as e:
        r.occluded(bad, sc.params(), out=out)
    assert e.value.code == T.TRT_ERR_INVALID
    assert (out == 0xA5).all()
    with pytest.raises(TrtError, match=r"segment 62 ") as e:
        r.occluded(bad[1:], sc.params(), out=out)  # record 63 is the lowest bad one of what was passed
    assert e.value.code == T.TRT_ERR_INVALID and (out == 0xA5).all()


# ---- 7: sizes and arguments ------------------------------------------------------------------------


def test_sizes_and_arguments(use, scenes, boundary):
    torch = pytest.importorskip("torch")
    sc = scenes["C3"]
    _, on, _, segs, idx = boundary["C3"]
    segs, idx = np.concatenate([segs, segs[::-1]])[:4099], np.concatenate([idx, idx[::-1]])[:4099]
    assert len(segs) == 4099
    want = expected_occluded(sc, segs, sc.flags, on[idx])
    r = use(sc)
    p = sc.params()
    dev = torch.from_numpy(segs.view(np.uint8).reshape(-1, 32)).to(f"cuda:{r.device}")
    for n in (0, 1, 63, 64, 65, 4099):
        out = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=dev.device)
        torch.cuda.synchronize(r.device)
        res = r.occluded(dev, p, out=out, nsegs=n)
        r.synchronize()
        assert res is out
        o = out.cpu().numpy()
        assert o[:n].tobytes() == want[:n].tobytes(), n
        assert (o[n:] == 0xA5).all(), n
        # the host path of the same size, into a padded array
        ho = np.full(n + 64, 0xA5, np.uint8)
        r.occluded(segs[:n], p, out=ho)
        assert ho[:n].tobytes() == want[:n].tobytes() and (ho[n:] == 0xA5).all(), n
    assert r.occluded(None, p).shape == (0,)  # nsegs == 0 is fine, and launches nothing
    # a device array is read as 16-byte vectors: an offset view is refused on the host, nothing runs
    raw = torch.zeros(32 * 8 + 16, dtype=torch.uint8, device=dev.device)
    off = raw[8:8 + 32 * 8]
    assert off.data_ptr() % 16 == 8
    out = torch.full((8,), 0xA5, dtype=torch.uint8, device=dev.device)
    torch.cuda.synchronize(r.device)
    with pytest.raises(TrtError, match="16-byte aligned") as e:
        r.occluded(off, p, out=out)
    assert e.value.code == T.TRT_ERR_INVALID
    r.synchronize()
    assert (out.cpu().numpy() == 0xA5).all()
    # the output needs no alignment
    odd = torch.full((64 + 3,), 0xA5, dtype=torch.uint8, device=dev.device)
    torch.cuda.synchronize(r.device)
    r.occluded(dev, p, out=odd[3:], nsegs=64)
    r.synchronize()
    o = odd.cpu().numpy()
    assert (o[:3] == 0xA5).all() and o[3:].tobytes() == want[:64].tobytes()
    with pytest.raises(TrtError) as e:  # any-hit counters are not offered
        r.occluded(segs, sc.params(flags=sc.flags | T.FLAG_COUNT))
    assert e.value.code == T.TRT_ERR_INVALID
    with pytest.raises(TrtError) as e:  # NULL segs
        r.occluded(None, p, nsegs=3)
    assert e.value.code == T.TRT_ERR_INVALID
    with Renderer(r.device) as fresh:
        with pytest.raises(TrtError) as e:
            fresh.occluded(segs[:4], p)
        assert e.value.code == T.TRT_ERR_NOSCENE


# ---- 8: streams and side effects --------------------------------------------------------------------


def test_query_on_a_torch_stream(use, scenes, boundary):
    torch = pytest.importorskip("torch")
    sc = scenes["C3"]
    segs = boundary["C3"][3][:1000]
    r = use(sc)
    p = sc.params()
    want = r.occluded(segs, p)
    dev = torch.from_numpy(segs.view(np.uint8).reshape(-1, 32)).to(f"cuda:{r.device}")
    torch.cuda.synchronize(r.device)
    s = torch.cuda.Stream(device=r.device)
    r.set_stream(s)
    try:
        with torch.cuda.stream(s):
            got = r.occluded(dev, p).cpu()  # on s, after the query
        s.synchronize()
    finally:
        r.set_stream(None)
    assert got.numpy().tobytes() == want.tobytes()
    timed, st = r.occluded(dev, p, timing=True)
    assert timed.cpu().numpy().tobytes() == want.tobytes() and st["kernel_ms"] > 0.0


def test_a_query_leaves_frames_and_ray_queries_as_they_were(use, scenes, boundary):
    torch = pytest.importorskip("torch")
    rays = random_rays(500, 9)
    for name in ("C2", "C3"):
        sc = scenes[name]
        segs = boundary[name][3]
        r = use(sc)
        p = sc.params()

        def state():
            frame, _, _ = r.draw_frame(p)
            _, _, hits, _ = r.trace_rays(rays, p, want8=False, want_hits=True)
            return frame.tobytes(), hits.tobytes()

        before = state()
        r.occluded(segs, p)
        r.occluded(segs, sc.params(flags=_no_floor(sc) | T.FLAG_BATCH_WALK))
        dev = torch.from_numpy(segs.view(np.uint8).reshape(-1, 32)).to(f"cuda:{r.device}")
        torch.cuda.synchronize(r.device)
        r.occluded(dev, p)
        r.synchronize()
        assert state() == before, name
