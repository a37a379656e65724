"""Visibility masks on the GPU (abi.h trt_visibility, visibility_query_kernel): the masks against the
CPU oracle, the identity mask bit == occluded(point_segments(...)) at every packing of points into a
wave, every mesh path and the adversarial meshes, bad points that share a wave with good ones, the
TARGETS edges (a point on its target, the range cap at a hit distance), arguments, sizes, streams and
side effects.  Every mask is compared exactly.  None of these provokes a fault: a bad record is inert
by contract and a misaligned call is refused on the host."""
from __future__ import annotations

import numpy as np
import pytest

from tests import mesh_cases as M
from tests.occlusion_common import expected_occluded, hits_for
from tests.query_common import f32, random_rays
from vkcomputeshader_tinyraytracer_amd import Renderer, TrtError, scene as S, types as T

pytestmark = pytest.mark.gpu

W, H = 71, 41
INF32 = f32(np.inf)
BAD = [0, 7, 8, 129]
NSETS = (1, 2, 3, 4, 7, 8, 9, 31, 32, 33, 63)


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


@pytest.fixture(scope="module")
def coop(gpu_renderer):
    """A context created under TRT_VIS_COOP=1: its GEOM 3 visibility kernel is the instantiation that
    may take the wave-cooperative shadow walk (with 33..63 entries a wave is one point, one origin:
    it always does on a quantized BVH).  The default context's lanes walk alone."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("TRT_VIS_COOP", "1")
        made = Renderer(gpu_renderer.device)
    try:
        yield made
    finally:
        made.close()


def on(ctx, sc):
    """A side context (g2, coop) with `sc` uploaded."""
    if ctx.scene is not sc:
        ctx.upload_scene(sc)
    return ctx


def _no_floor(sc) -> int:
    return int(sc.flags) & ~T.FLAG_FLOOR


def pack(occ, npts: int, nset: int) -> np.ndarray:
    """(npts * nset) occlusion bytes, [i * nset + k], as (npts,) uint64 masks, bit k = byte (i, k)."""
    occ = np.asarray(occ).reshape(npts, nset)
    assert np.isin(occ, (T.OCC_VISIBLE, T.OCC_OCCLUDED)).all()
    bits = (occ == T.OCC_OCCLUDED).astype(np.uint64) << np.arange(nset, dtype=np.uint64)[None]
    return np.bitwise_or.reduce(bits, axis=1) if nset else np.zeros(npts, np.uint64)


def to_device(torch, recs, device):
    t = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1, 32)).to(f"cuda:{device}")
    torch.cuda.synchronize(device)
    return t


def masks_of(r, tensor) -> np.ndarray:
    r.synchronize()
    return tensor.cpu().numpy().view(np.uint64)


def lights_of(sc) -> np.ndarray:
    return np.array([sc.ubo[f"light{i}"][:3] for i in range(3)], f32).reshape(3, 3)


def with_tmax(points, tmax):
    p = points.copy()
    p["tmax"] = tmax
    return p


# ---- the point set ---------------------------------------------------------------------------------


def aimed_rays(n: int) -> np.ndarray:
    """tests/test_gpu_occlusion.py's aimed_rays recipe at n rays: random_rays(n, 4242) with every
    second ray starting near the mesh and aimed at it."""
    rays = random_rays(n, 4242)
    rng = np.random.default_rng(99)
    aim = np.arange(0, len(rays), 2)
    rays["org"][aim] = (np.array((2.5, -2.0, -10.0)) + rng.uniform(-4, 4, size=(len(aim), 3))).astype(f32)
    rays["dir"][aim] = (np.array((2.5, -2.0, -10.0)) + rng.uniform(-1.2, 1.2, size=(len(aim), 3)) - rays["org"][aim]).astype(f32)
    return rays


def free_points(n: int, seed: int) -> np.ndarray:
    rays = random_rays(n, seed)
    p = np.zeros(n, T.QPOINT)
    p["pos"], p["n"], p["tmax"] = rays["org"], rays["dir"], T.QSEG_MAX_T
    return p


@pytest.fixture(scope="module")
def points(scenes):
    """128 points: the first 96 hits (the oracle's records on C3) of aimed_rays(257) through
    points_on_hits, plus 32 free points with origin and dir-as-normal of random_rays(32, 5)."""
    sc = scenes["C3"]
    rays = aimed_rays(257)
    hits = hits_for(sc, rays, sc.flags)
    on, _ = S.points_on_hits(rays, hits)
    assert len(on) >= 96 and int((hits["kind"] == T.HIT_TRIANGLE).sum()) > 20
    pts = np.concatenate([on[:96], free_points(32, 5)])
    assert len(pts) == 128 and S.lib().trt_check_points(pts.ctypes.data, 128, None) == 0
    return pts


# ---- 1: against the oracle -----------------------------------------------------------------------

ORACLE_CASES = [("C3", True, 63, 2.0), ("C3", True, 16, 1e10), ("C3", True, 5, 0.75), ("C3", False, 16, 1e10),
                ("C2", True, 63, 2.0)]


@pytest.fixture(scope="module")
def oracle_refs(scenes, points):
    """Per case: the points, the directions and the oracle's masks — computed once, before the GPU
    is asked, with the conditions that make the case worth asking."""
    out = {}
    for name, floor, nset, tmax in ORACLE_CASES:
        sc = scenes[name]
        flags = sc.flags if floor else _no_floor(sc)
        pts = with_tmax(points, f32(tmax))
        dirs = S.sphere_dirs(nset)
        segs = S.point_segments(pts, dirs=dirs)
        want = pack(expected_occluded(sc, segs, flags), len(pts), nset)
        full = np.uint64((1 << nset) - 1)
        mixed = int(((want != 0) & (want != full)).sum())
        flipped = (segs["dir"] != dirs[None]).any(-1)
        assert mixed >= 8, (name, floor, nset, tmax, mixed)
        assert flipped.any() and not flipped.all()
        out[(name, floor, nset, tmax)] = (pts, dirs, want, mixed)
    return out


@pytest.mark.parametrize("name,floor,nset,tmax", ORACLE_CASES,
                         ids=[f"{n}-{'floor' if f else 'nofloor'}-{k}x{t:g}" for n, f, k, t in ORACLE_CASES])
def test_dirs_against_the_oracle(use, coop, scenes, oracle_refs, name, floor, nset, tmax):
    sc = scenes[name]
    pts, dirs, want, mixed = oracle_refs[(name, floor, nset, tmax)]
    r = use(sc)
    got = r.visibility(pts, sc.params(flags=sc.flags if floor else _no_floor(sc)), dirs=dirs)
    assert got.dtype == np.uint64 and got.shape == (len(pts),)
    print(f"{name} floor={floor} {nset} x tmax {tmax:g}: {mixed} mixed masks, {int((got != want).sum())} of {len(want)} differ")
    assert got.tobytes() == want.tobytes()
    # the same through the cooperative instantiation
    again = on(coop, sc).visibility(pts, sc.params(flags=sc.flags if floor else _no_floor(sc)), dirs=dirs)
    assert again.tobytes() == want.tobytes()


@pytest.mark.parametrize("floor", [True, False], ids=["floor", "nofloor"])
def test_targets_against_the_oracle(use, scenes, points, floor):
    sc = scenes["C3"]
    flags = sc.flags if floor else _no_floor(sc)
    lights = lights_of(sc)
    between = S.segments_between(points["pos"][:, None, :], lights[None])
    want = pack(expected_occluded(sc, between.reshape(-1), flags), len(points), 3)
    seen = sorted(set(want.tolist()))
    print(f"floor={floor}: light patterns {seen}")
    assert seen == list(range(8))  # every pattern of the three lights
    r = use(sc)
    got = r.visibility(points, sc.params(flags=flags), targets=lights)
    assert got.tobytes() == want.tobytes()
    four = np.concatenate([lights, np.full((3, 1), np.nan, f32)], 1)  # the fourth float is ignored
    assert r.visibility(points, sc.params(flags=flags), targets=four).tobytes() == want.tobytes()


# ---- 2: the identity on the GPU, every packing ---------------------------------------------------------


@pytest.fixture(scope="module")
def thousand(gpu_renderer, scenes):
    """1,000 points on C3: the hits (the GPU's own records) of random_rays(1500, 77) through
    points_on_hits, filled up with free points; tmax mixed over the three ranges of the oracle cases."""
    sc = scenes["C3"]
    r = gpu_renderer
    r.upload_scene(sc)
    rays = random_rays(1500, 77)
    _, _, hits, _ = r.trace_rays(rays, sc.params(), want8=False, want_hits=True)
    on, _ = S.points_on_hits(rays, hits)
    assert 200 < len(on) < 1000
    pts = np.concatenate([on, free_points(1000 - len(on), 12)])
    pts["tmax"] = np.random.default_rng(4).choice(np.array((0.75, 2.0, 1e10), f32), 1000)
    return pts


@pytest.mark.parametrize("nset", NSETS)
def test_identity_at_every_packing(use, coop, scenes, thousand, nset):
    """L = 1, 2, 4, 4, 8, 8, 16, 32, 32, 64, 64 lanes per point.  1,000 points end in a ragged wave
    at L <= 4 and at 64 / L = 1; 999 points do at every L < 64.  Both tails must be right."""
    sc = scenes["C3"]
    r = use(sc)
    p = sc.params()
    dirs = S.sphere_dirs(nset)
    want = pack(r.occluded(S.point_segments(thousand, dirs=dirs).reshape(-1), p), 1000, nset)
    assert (want != 0).any() and (want >> np.uint64(nset) == 0).all()
    got = r.visibility(thousand, p, dirs=dirs)
    print(f"nset {nset}: {int((got != want).sum())} of 1000 differ, tail mask {int(want[-1]):#x}")
    assert got[-1] == want[-1]
    assert got.tobytes() == want.tobytes()
    out = np.full(1000, 0xA5A5A5A5A5A5A5A5, np.uint64)
    r.visibility(thousand, p, dirs=dirs, out=out, npoints=999)
    assert out[998] == want[998] and out[:999].tobytes() == want[:999].tobytes() and out[999] == 0xA5A5A5A5A5A5A5A5
    assert on(coop, sc).visibility(thousand, p, dirs=dirs).tobytes() == want.tobytes()  # the cooperative instantiation


# ---- 3: mesh paths ------------------------------------------------------------------------------------


def test_every_mesh_path(use, scenes, oracle_refs, g2, coop):
    """The default quantized BVH (GEOM 3, every lane walking alone), the same with the
    wave-cooperative walk allowed (a TRT_VIS_COOP=1 context), the reference-order batch walk
    (TRT_FLAG_BATCH_WALK, GEOM 1) and the unquantized BVH of a TRT_BVH_WAVES4=0 context (GEOM 2): 48
    points x 16 directions, equal to the oracle's masks and to each other."""
    sc = scenes["C3"]
    pts, dirs, want, _ = oracle_refs[("C3", True, 16, 1e10)]
    pts, want = pts[:48], want[:48]
    assert (want != 0).any() and (want != 0xFFFF).any()
    r = use(sc)
    a = r.visibility(pts, sc.params(), dirs=dirs)
    b = r.visibility(pts, sc.params(flags=sc.flags | T.FLAG_BATCH_WALK), dirs=dirs)
    c = on(g2, sc).visibility(pts, sc.params(), dirs=dirs)
    d = on(coop, sc).visibility(pts, sc.params(), dirs=dirs)
    for path, got in (("GEOM 3", a), ("GEOM 1", b), ("GEOM 2", c), ("GEOM 3 cooperative", d)):
        assert got.tobytes() == want.tobytes(), path


def _points_on_triangles(sc, seed: int, n: int = 48) -> np.ndarray:
    """n points 1e-3 off triangles drawn from the mesh (of those within 100 units that have an
    area), at a point drawn inside each, the triangle's normal as n."""
    rng = np.random.default_rng(seed)
    v = np.stack([sc.tris[k][:, :3] for k in ("v0", "v1", "v2")], 1).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        cr = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        area = np.linalg.norm(cr, axis=1)
    big = np.flatnonzero((area > 1e-3) & (np.abs(v).max(axis=(1, 2)) < 100.0))
    pick = rng.choice(big, n)
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    nrm = cr[pick] / area[pick][:, None]
    p = np.zeros(n, T.QPOINT)
    p["pos"] = np.einsum("nk,nkc->nc", w, v[pick]) + 1e-3 * nrm
    p["n"] = nrm
    p["tmax"] = T.QSEG_MAX_T
    return p


@pytest.fixture(scope="module")
def adversarial():
    out = {}
    dirs = S.sphere_dirs(16)
    for i, name in enumerate(M.QUERY_CASES):
        sc = M.CASES[name].scene
        pts = _points_on_triangles(sc, 8100 + i)
        want = pack(expected_occluded(sc, S.point_segments(pts, dirs=dirs), sc.flags), len(pts), 16)
        assert (want != 0).any() and (want != 0xFFFF).any(), name
        out[name] = (pts, want)
    return out


@pytest.mark.parametrize("name", M.QUERY_CASES)
def test_adversarial_meshes(use, g2, coop, adversarial, name):
    sc = M.CASES[name].scene
    pts, want = adversarial[name]
    dirs = S.sphere_dirs(16)
    r = use(sc)
    a = r.visibility(pts, sc.params(), dirs=dirs)
    b = r.visibility(pts, sc.params(flags=sc.flags | T.FLAG_BATCH_WALK), dirs=dirs)
    c = on(g2, sc).visibility(pts, sc.params(), dirs=dirs)
    d = on(coop, sc).visibility(pts, sc.params(), dirs=dirs)
    for path, got in (("default", a), ("batch walk", b), ("TRT_BVH_WAVES4=0", c), ("TRT_VIS_COOP=1", d)):
        print(f"{name} {path}: {int((got != want).sum())} of {len(want)} differ")
        assert got.tobytes() == want.tobytes(), path


# ---- 4: bad points share waves ----------------------------------------------------------------------------


@pytest.mark.parametrize("nset", [5, 63])
def test_bad_points_share_waves_with_good_ones(use, coop, scenes, points, nset):
    """At nset = 5 a wave holds 8 points: points 0 and 7 share the first wave with six good ones,
    point 8 opens the second, point 129 sits in the ragged last one.  At 63 each has a wave."""
    torch = pytest.importorskip("torch")
    sc = scenes["C3"]
    good = with_tmax(np.concatenate([points, free_points(2, 6)]), f32(2.0))
    assert len(good) == 130
    bad = good.copy()
    bad["pos"][0, 1] = np.nan
    bad["n"][7, 2] = np.inf
    bad["tmax"][8] = 0.0
    bad["tmax"][129] = np.nan
    r = use(sc)
    p = sc.params()
    dirs = S.sphere_dirs(nset)
    host = r.visibility(good, p, dirs=dirs)
    assert (host != 0).any() and (host != np.uint64(T.VIS_BAD_POINT)).all()
    got = r.visibility(to_device(torch, bad, r.device), p, dirs=dirs)
    assert got.dtype == torch.int64 and got.shape == (130,) and got.is_cuda
    r.synchronize()
    assert (got.cpu().numpy()[BAD] == -1).all()
    got = masks_of(r, got)
    rest = np.setdiff1d(np.arange(130), BAD)
    assert (got[BAD] == np.uint64(T.VIS_BAD_POINT)).all()
    assert got[rest].tobytes() == host[rest].tobytes()
    # the good array from the device: the same bytes as through host pointers
    again = masks_of(r, r.visibility(to_device(torch, good, r.device), p, dirs=dirs))
    assert again.tobytes() == host.tobytes()
    # the cooperative instantiation, entered by whatever lanes the bad points leave
    cgot = masks_of(coop, on(coop, sc).visibility(to_device(torch, bad, coop.device), p, dirs=dirs))
    assert (cgot[BAD] == np.uint64(T.VIS_BAD_POINT)).all() and cgot[rest].tobytes() == host[rest].tobytes()
    # and in TARGETS mode
    lights = lights_of(sc)
    thost = r.visibility(good, p, targets=lights)
    tgot = masks_of(r, r.visibility(to_device(torch, bad, r.device), p, targets=lights))
    assert (tgot[BAD] == np.uint64(T.VIS_BAD_POINT)).all() and tgot[rest].tobytes() == thost[rest].tobytes()


# ---- 5: TARGETS edges -----------------------------------------------------------------------------------------


def test_a_point_on_its_target_sees_it(use, scenes, points):
    torch = pytest.importorskip("torch")
    sc = scenes["C3"]
    lights = lights_of(sc)
    pts = points[:9].copy()
    pts["pos"][4] = lights[0]
    between = S.segments_between(pts["pos"][:, None, :], lights[None])
    ok = np.ones((9, 3), bool)
    ok[4, 0] = False  # a zero direction: not a valid segment, not traced, reads 0
    want = np.zeros((9, 3), np.uint8)
    want[ok] = expected_occluded(sc, between[ok], sc.flags)
    want = pack(want, 9, 3)
    r = use(sc)
    got = r.visibility(pts, sc.params(), targets=lights)
    assert got[4] & np.uint64(1) == 0
    assert got.tobytes() == want.tobytes()
    dev = masks_of(r, r.visibility(to_device(torch, pts, r.device), sc.params(), targets=lights))
    assert dev.tobytes() == want.tobytes()  # host and device arrays alike


def test_the_range_cap_at_a_hit_distance(use, scenes, points):
    """tmax caps the range to a target: a cap at an occluder's own distance t clears its bit (the
    test is strict), the next float sets it.  t is the GPU's own hit record of the ray the kernel
    forms (dir = light - pos)."""
    sc = scenes["C3"]
    lights = lights_of(sc)
    r = use(sc)
    p = sc.params()
    full = r.visibility(points, p, targets=lights)
    for k in range(3):
        seg = S.segments_between(points["pos"], lights[k])
        rays = np.zeros(len(points), T.QRAY)
        rays["org"], rays["dir"] = seg["org"], seg["dir"]
        _, _, hits, _ = r.trace_rays(rays, p, want8=False, want_hits=True)
        blocked = hits["t"] < seg["tmax"]
        bit = (full >> np.uint64(k)) & np.uint64(1)
        assert bit.tobytes() == blocked.astype(np.uint64).tobytes()
        assert blocked.sum() >= 8, k
        t = np.where(blocked, hits["t"], T.QSEG_MAX_T).astype(f32)
        at = r.visibility(with_tmax(points, t), p, targets=lights)
        after = r.visibility(with_tmax(points, np.where(blocked, np.nextafter(t, INF32), T.QSEG_MAX_T).astype(f32)), p,
                             targets=lights)
        assert (((at >> np.uint64(k)) & np.uint64(1))[blocked] == 0).all(), k
        assert (((after >> np.uint64(k)) & np.uint64(1))[blocked] == 1).all(), k
        assert (((at >> np.uint64(k)) & np.uint64(1))[~blocked] == 0).all(), k


# ---- 6: arguments ------------------------------------------------------------------------------------------------


def test_host_rejection(use, scenes, points):
    sc = scenes["C3"]
    r = use(sc)
    dirs = S.sphere_dirs(5)
    bad = points.copy()
    bad["tmax"][9] = np.nan
    bad["pos"][3, 0] = np.inf
    out = np.full(128, 0xA5A5A5A5A5A5A5A5, np.uint64)
    with pytest.raises(TrtError, match=r"point 3 ") as e:
        r.visibility(bad, sc.params(), dirs=dirs, out=out)
    assert e.value.code == T.TRT_ERR_INVALID and (out == 0xA5A5A5A5A5A5A5A5).all()
    with pytest.raises(TrtError, match=r"point 5 ") as e:
        r.visibility(bad[4:], sc.params(), dirs=dirs, out=out)  # record 9 is the lowest bad one of what was passed
    assert e.value.code == T.TRT_ERR_INVALID and (out == 0xA5A5A5A5A5A5A5A5).all()
    zero = dirs.copy()
    zero[2] = 0.0
    with pytest.raises(TrtError, match=r"set entry 2 ") as e:
        r.visibility(points, sc.params(), dirs=zero, out=out)
    assert e.value.code == T.TRT_ERR_INVALID and (out == 0xA5A5A5A5A5A5A5A5).all()
    assert r.visibility(points, sc.params(), targets=zero).shape == (128,)  # the origin is a fine target


def test_sizes_and_arguments(use, scenes, thousand):
    torch = pytest.importorskip("torch")
    sc = scenes["C3"]
    r = use(sc)
    p = sc.params()
    pts = np.concatenate([thousand, thousand[::-1], thousand, thousand[::-1], thousand])[:4099]
    assert len(pts) == 4099
    dirs = S.sphere_dirs(3)
    want = pack(r.occluded(S.point_segments(pts, dirs=dirs).reshape(-1), p), 4099, 3)
    dev = to_device(torch, pts, r.device)
    for n in (0, 1, 63, 64, 65, 4099):
        out = torch.full((n + 8,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev.device)
        torch.cuda.synchronize(r.device)
        res = r.visibility(dev, p, dirs=dirs, out=out, npoints=n)
        assert res is out
        o = masks_of(r, out)
        assert o[:n].tobytes() == want[:n].tobytes(), n
        assert (o[n:] == 0xA5A5A5A5A5A5A5A5).all(), n
        ho = np.full(n + 8, 0xA5A5A5A5A5A5A5A5, np.uint64)  # the host path of the same size
        r.visibility(pts[:n], p, dirs=dirs, out=ho)
        assert ho[:n].tobytes() == want[:n].tobytes() and (ho[n:] == 0xA5A5A5A5A5A5A5A5).all(), n
    assert r.visibility(None, p, dirs=dirs).shape == (0,)  # npts == 0 is fine, and launches nothing
    # refused on the host, nothing runs: the set's size, both or neither set, misaligned device arrays, COUNT
    out = np.full(8, 0xA5A5A5A5A5A5A5A5, np.uint64)
    for k in (0, 64):
        with pytest.raises(TrtError) as e:
            r.visibility(pts[:8], p, dirs=np.tile(dirs, (22, 1))[:k].reshape(k, 3), out=out)
        assert e.value.code == T.TRT_ERR_INVALID and (out == 0xA5A5A5A5A5A5A5A5).all(), k
    with pytest.raises(ValueError):
        r.visibility(pts[:8], p)
    with pytest.raises(ValueError):
        r.visibility(pts[:8], p, dirs=dirs, targets=dirs)
    raw = torch.zeros(32 * 8 + 16, dtype=torch.uint8, device=dev.device)
    off = raw[8:8 + 32 * 8]
    assert off.data_ptr() % 16 == 8
    dout = torch.full((8,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev.device)
    torch.cuda.synchronize(r.device)
    with pytest.raises(TrtError, match="16-byte aligned") as e:
        r.visibility(off, p, dirs=dirs, out=dout)
    assert e.value.code == T.TRT_ERR_INVALID
    oraw = torch.full((8 * 8 + 8,), 0xA5, dtype=torch.uint8, device=dev.device)
    assert oraw[4:].data_ptr() % 8 == 4
    torch.cuda.synchronize(r.device)
    with pytest.raises(TrtError, match="8-byte aligned") as e:
        r.visibility(dev, p, dirs=dirs, out=oraw[4:], npoints=8)
    assert e.value.code == T.TRT_ERR_INVALID
    r.synchronize()
    assert (masks_of(r, dout) == 0xA5A5A5A5A5A5A5A5).all() and (oraw.cpu().numpy() == 0xA5).all()
    with pytest.raises(TrtError) as e:  # any-hit counters are not offered
        r.visibility(pts[:8], sc.params(flags=sc.flags | T.FLAG_COUNT), dirs=dirs)
    assert e.value.code == T.TRT_ERR_INVALID
    with pytest.raises(TrtError) as e:  # NULL pts
        r.visibility(None, p, dirs=dirs, npoints=3)
    assert e.value.code == T.TRT_ERR_INVALID
    with Renderer(r.device) as fresh:
        with pytest.raises(TrtError) as e:
            fresh.visibility(pts[:4], p, dirs=dirs)
        assert e.value.code == T.TRT_ERR_NOSCENE


# ---- 7: streams and side effects -------------------------------------------------------------------------------------


def test_query_on_a_torch_stream(use, scenes, thousand):
    torch = pytest.importorskip("torch")
    sc = scenes["C3"]
    r = use(sc)
    p = sc.params()
    dirs = S.sphere_dirs(16)
    want = r.visibility(thousand, p, dirs=dirs)
    dev = to_device(torch, thousand, r.device)
    s = torch.cuda.Stream(device=r.device)
    r.set_stream(s)
    try:
        with torch.cuda.stream(s):
            got = r.visibility(dev, p, dirs=dirs).cpu()  # on s, after the query
        s.synchronize()
    finally:
        r.set_stream(None)
    assert got.numpy().view(np.uint64).tobytes() == want.tobytes()
    timed, st = r.visibility(dev, p, dirs=dirs, timing=True)
    assert timed.cpu().numpy().view(np.uint64).tobytes() == want.tobytes() and st["kernel_ms"] > 0.0


def test_a_query_leaves_frames_and_other_queries_as_they_were(use, scenes, points):
    torch = pytest.importorskip("torch")
    rays = random_rays(500, 9)
    segs = S.segments_from_rays(rays, 6.0)
    for name in ("C2", "C3"):
        sc = scenes[name]
        r = use(sc)
        p = sc.params()

        def state():
            frame, _, _ = r.draw_frame(p)
            _, _, hits, _ = r.trace_rays(rays, p, want8=False, want_hits=True)
            return frame.tobytes(), hits.tobytes(), r.occluded(segs, p).tobytes()

        before = state()
        r.visibility(points, p, dirs=S.sphere_dirs(63))
        r.visibility(points, sc.params(flags=_no_floor(sc) | T.FLAG_BATCH_WALK), targets=lights_of(sc))
        r.visibility(to_device(torch, points, r.device), p, dirs=S.sphere_dirs(5))
        r.synchronize()
        assert state() == before, name
