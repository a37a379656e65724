"""All-hits queries on the GPU (abi.h trt_trace_all, all_hits_kernel): every record and count exact
against the oracle's reference (tests/allhits_common.py), the identities with trace_rays and occluded
on the GPU's own answers, every mesh path, the adversarial meshes (split duplicates, coincident
triangles, the fallback walk), bad records in a device array, sizes, arguments, streams, side effects
and Renderer.contains.  Every comparison of counts and of t / kind / index / n is byte for byte.  None
of these provokes a fault: a bad record is inert by contract and a bad call is refused on the host."""
from __future__ import annotations

import numpy as np
import pytest

from tests import allhits_common as AH
from tests import mesh_cases as M
from tests.query_common import f32, normalize32, random_rays
from tests.test_gpu_occlusion import _query_rays, aimed_rays
from vkcomputeshader_tinyraytracer_amd import Renderer, TrtError, scene as S, types as T

pytestmark = pytest.mark.gpu

W, H = 71, 41
BAD = [0, 63, 64, 129]
KS = (1, 4, 32)
CNT = 0x7FFFFFFF


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
    """A context created under TRT_BVH_WAVES4=0: mesh scenes take the GEOM 2 kernels."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("TRT_BVH_WAVES4", "0")
        made = Renderer(gpu_renderer.device)
    try:
        yield made
    finally:
        made.close()


def _no_floor(sc) -> int:
    return int(sc.flags) & ~T.FLAG_FLOOR


def drop_floor(cands):
    """The candidates of the same query without TRT_FLAG_FLOOR: the candidates are independent
    primitive tests, so the list without the floor is the list with it less its floor record."""
    return [[r for r in c if r[4] != T.HIT_FLOOR] for c in cands]


def as_records(hits, n, k):
    """A device query's (n, K, 32) uint8 tensor as (n, K) T.QHIT."""
    return np.ascontiguousarray(hits.cpu().numpy()).view(T.QHIT).reshape(n, k)


def to_dev(torch, r, segs):
    dev = torch.from_numpy(np.ascontiguousarray(segs).view(np.uint8).reshape(-1, 32)).to(f"cuda:{r.device}")
    torch.cuda.synchronize(r.device)
    return dev


def check_answer(sc, segs, got, want):
    """counts byte for byte; t, kind, index, n of every slot byte for byte; slots past the count are
    the miss record; u, v are zero off triangles and the barycentric point is the hit point on them."""
    (gh, gc), (wh, wc) = got, want
    assert gc.dtype == np.uint32 and gh.dtype == T.QHIT and gh.shape == wh.shape
    assert gc.tobytes() == wc.tobytes()
    AH.same_records(gh, wh)
    nontri = gh[gh["kind"] != T.HIT_TRIANGLE]
    assert not nontri["u"].any() and not nontri["v"].any()
    past = np.arange(gh.shape[1])[None, :] >= (gc & CNT)[:, None]
    assert gh[past].tobytes() == np.tile(AH.MISS, int(past.sum())).tobytes()
    d = normalize32(segs["dir"]).astype(np.float64)
    for i, j in zip(*np.nonzero(gh["kind"] == T.HIT_TRIANGLE)):
        h = gh[i, j]
        tr, u, v = sc.tris[h["index"]], float(h["u"]), float(h["v"])
        pb = (1 - u - v) * tr["v0"][:3].astype(np.float64) + u * tr["v1"][:3] + v * tr["v2"][:3]
        pr = segs["org"][i].astype(np.float64) + d[i] * float(h["t"])
        assert np.abs(pb - pr).max() <= 1e-4 * max(1.0, np.abs(pr).max()), (i, j, pb, pr)


# ---- 1: exact against the reference -------------------------------------------------------------


@pytest.fixture(scope="module")
def refs(scenes):
    """Per scene: whole-ray segments (C2: random_rays(2053, 77); C3: the aimed set) and the
    reference's candidate lists with the floor and without it."""
    out = {}
    for name, rays in (("C2", random_rays(2053, 77)), ("C3", aimed_rays())):
        sc = scenes[name]
        segs = S.segments_from_rays(rays)
        on = AH.all_candidates(sc, segs, sc.flags)
        tot = AH.totals(on)
        kinds = {r[4] for c in on for r in c}
        assert (tot == 0).any() and (tot > 4).any() and tot.max() <= 32, tot.max()
        assert {T.HIT_FLOOR, T.HIT_SPHERE} <= kinds and (name == "C2" or T.HIT_TRIANGLE in kinds)
        out[name] = (segs, {True: on, False: drop_floor(on)})
    return out


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("floor", [True, False], ids=["floor", "nofloor"])
@pytest.mark.parametrize("name", ["C2", "C3"])
def test_exact_against_the_reference(use, scenes, refs, name, floor, k):
    sc = scenes[name]
    segs, cands = refs[name]
    flags = int(sc.flags) if floor else _no_floor(sc)
    want = AH.records(cands[floor], k)
    r = use(sc)
    got = r.trace_all(segs, sc.params(flags=flags), k)
    assert got[0].shape == (len(segs), k)
    more = int(((want[1] & T.ALLHITS_MORE) != 0).sum())
    print(f"{name} floor={floor} K={k}: {int((want[1] & CNT).sum())} records, {more} truncated, "
          f"{int((got[1] != want[1]).sum())} counts differ")
    assert (k == 32) == (more == 0)
    check_answer(sc, segs, got, want)


# ---- 2: the identities, on the GPU's own answers ---------------------------------------------------


def test_identities(use, scenes, refs):
    sc = scenes["C3"]
    segs, _ = refs["C3"]
    r = use(sc)
    p = sc.params()
    h32, c32 = r.trace_all(segs, p, 32)
    assert not (c32 & T.ALLHITS_MORE).any()
    # record 0 is the trace_rays record, all 32 bytes (whole rays: every record's t < tmax or a miss)
    rays = AH.rays_of(segs)
    _, _, first, _ = r.trace_rays(rays, p, want8=False, want_hits=True)
    assert np.ascontiguousarray(h32[:, 0]).tobytes() == first.tobytes()
    # a count above zero is occluded's byte
    occ = r.occluded(segs, p)
    assert ((c32 > 0).astype(np.uint8)).tobytes() == occ.tobytes() and occ.any() and not occ.all()
    # K = 4 is the prefix of K = 32, with MORE exactly where the total exceeds 4
    h4, c4 = r.trace_all(segs, p, 4)
    assert h4.tobytes() == np.ascontiguousarray(h32[:, :4]).tobytes()
    assert ((c4 & CNT) == np.minimum(c32, 4)).all() and (((c4 & T.ALLHITS_MORE) != 0) == (c32 > 4)).all()
    assert (c32 > 4).any()
    # counts only: the same counts, at both sizes
    none, c4b = r.trace_all(segs, p, 4, want_hits=False)
    assert none is None and c4b.tobytes() == c4.tobytes()
    assert r.trace_all(segs, p, 32, want_hits=False)[1].tobytes() == c32.tobytes()
    # cut off at the t of record j: exactly the records with a smaller t (tmax is strict)
    sel, tm = [], []
    for i in np.flatnonzero(c32 >= 2):
        for j in {1, int(c32[i]) - 1}:
            sel.append(i)
            tm.append(h32[i, j]["t"])
    sel, tm = np.asarray(sel), np.asarray(tm, f32)
    assert len(sel) > 100
    cut = segs[sel].copy()
    cut["tmax"] = tm
    hc, cc = r.trace_all(cut, p, 32)
    below = h32[sel]["t"] < tm[:, None]
    below &= np.arange(32)[None, :] < c32[sel][:, None]
    assert cc.tobytes() == below.sum(1).astype(np.uint32).tobytes()
    want = np.tile(AH.MISS, (len(sel), 32))
    want[below] = h32[sel][below]  # a prefix: the records are in order of t
    assert (below[:, 1:] <= below[:, :-1]).all()
    assert hc.tobytes() == want.tobytes()
    # and record 0 against trace_rays where the ray's record lies beyond tmax: nothing is reported
    beyond = first["t"][sel] >= tm
    assert (cc[beyond] == 0).all()


# ---- 3: every mesh path ----------------------------------------------------------------------------


def three_paths(r, g2, sc, segs, k, flags=None):
    flags = int(sc.flags) if flags is None else flags
    a = r.trace_all(segs, sc.params(flags=flags), k)
    b = r.trace_all(segs, sc.params(flags=flags | T.FLAG_BATCH_WALK), k)
    g2.upload_scene(sc)
    c = g2.trace_all(segs, sc.params(flags=flags), k)
    return (("default", a), ("batch walk", b), ("TRT_BVH_WAVES4=0", c))


def test_every_mesh_path(use, scenes, refs, g2):
    """The default quantized BVH (GEOM 3), the reference-order batch walk (GEOM 1) and the unquantized
    BVH of a TRT_BVH_WAVES4=0 context (GEOM 2): equal to the reference and, whole records, to each other."""
    sc = scenes["C3"]
    segs, cands = refs["C3"]
    want = AH.records(cands[True], 32)
    got = three_paths(use(sc), g2, sc, segs, 32)
    for path, ans in got:
        check_answer(sc, segs, ans, want)
        assert ans[0].tobytes() == got[0][1][0].tobytes(), path


# ---- 4: adversarial meshes ---------------------------------------------------------------------------

CASES4 = M.QUERY_CASES + ("many_models_b7",)


@pytest.fixture(scope="module")
def adversarial():
    out = {}
    for i, name in enumerate(CASES4):
        sc = M.CASES[name].scene
        segs = S.segments_from_rays(_query_rays(sc, 7000 + i))
        cands = AH.all_candidates(sc, segs, sc.flags)
        tot = AH.totals(cands)
        assert tot.max() <= 32 and (tot >= 2).sum() > 50, (name, tot.max())
        out[name] = (segs, cands)
    # conditions on the inputs: the ties and the deep counts exist without construction
    assert AH.equal_t_pairs(out["degenerate_mix"][1]) > 0
    assert AH.totals(out["soup_loguniform"][1]).max() > 8
    return out


@pytest.mark.parametrize("name", CASES4)
def test_adversarial_meshes(use, g2, adversarial, name):
    sc = M.CASES[name].scene
    segs, cands = adversarial[name]
    want = AH.records(cands, 32)
    got = three_paths(use(sc), g2, sc, segs, 32)
    for path, ans in got:
        print(f"{name} {path}: {int((ans[1] != want[1]).sum())} of {len(segs)} counts differ, max {int(want[1].max())}")
        check_answer(sc, segs, ans, want)
    if name == "soup_loguniform":  # truncated at 8: the prefix and the MORE bit
        h8, c8 = use(sc).trace_all(segs, sc.params(), 8)
        w8 = AH.records(cands, 8)
        assert (w8[1] & T.ALLHITS_MORE).any()
        check_answer(sc, segs, (h8, c8), w8)


# ---- 5: bad records in a device array ---------------------------------------------------------------


@pytest.fixture(scope="module")
def ragged(refs):
    good = refs["C3"][0][:130].copy()
    bad = good.copy()
    bad["dir"][0] = (np.nan, 0.0, -1.0)
    bad["dir"][63] = 0.0
    bad["org"][64, 1] = np.inf
    bad["tmax"][129] = np.nan
    return good, bad


def test_bad_records_in_a_device_array(use, scenes, ragged):
    torch = pytest.importorskip("torch")
    sc = scenes["C3"]
    good, bad = ragged
    r = use(sc)
    p = sc.params()
    K = 4
    hh, hc = r.trace_all(good, p, K)
    assert (hc & CNT).max() >= 3 and (hc == 0).any()
    rest = np.setdiff1d(np.arange(130), BAD)
    for want_hits in (True, False):
        hits, counts = r.trace_all(to_dev(torch, r, bad), p, K, want_hits=want_hits)
        r.synchronize()
        assert counts.dtype == torch.int32 and counts.shape == (130,) and counts.is_cuda
        c = counts.cpu().numpy().view(np.uint32)
        assert (c[BAD] == T.ALLHITS_BAD_SEG).all()
        assert c[rest].tobytes() == hc[rest].tobytes()
        if not want_hits:
            assert hits is None
            continue
        assert hits.dtype == torch.uint8 and hits.shape == (130, K, 32)
        h = as_records(hits, 130, K)
        marker = np.zeros(1, T.QHIT)
        marker["kind"] = T.HIT_BAD_RAY
        assert h[BAD].tobytes() == np.tile(marker, len(BAD) * K).tobytes()
        assert h[rest].tobytes() == hh[rest].tobytes()
    # the good array from the device: the same bytes as through host pointers
    hits, counts = r.trace_all(to_dev(torch, r, good), p, K)
    r.synchronize()
    assert as_records(hits, 130, K).tobytes() == hh.tobytes() and counts.cpu().numpy().view(np.uint32).tobytes() == hc.tobytes()


def test_host_rejection(use, scenes, ragged):
    sc = scenes["C3"]
    _, bad = ragged
    r = use(sc)
    hits = np.zeros((130, 4), T.QHIT)
    hits.view(np.uint8)[:] = 0xA5
    counts = np.full(130, 0xA5A5A5A5, np.uint32)
    with pytest.raises(TrtError, match=r"segment 0 ") as e:
        r.trace_all(bad, sc.params(), 4, hits=hits, counts=counts)
    assert e.value.code == T.TRT_ERR_INVALID
    with pytest.raises(TrtError, match=r"segment 62 ") as e:
        r.trace_all(bad[1:], sc.params(), 4, hits=hits, counts=counts)  # record 63 is the lowest bad one passed
    assert e.value.code == T.TRT_ERR_INVALID
    assert (hits.view(np.uint8) == 0xA5).all() and (counts == 0xA5A5A5A5).all()


# ---- 6: sizes, arguments, streams, side effects -------------------------------------------------------


def test_sizes_and_arguments(use, scenes, refs):
    torch = pytest.importorskip("torch")
    sc = scenes["C3"]
    segs, cands = refs["C3"]
    assert len(segs) == 1027
    K = 4
    wh, wc = AH.records(cands[True], K)
    r = use(sc)
    p = sc.params()
    dev = to_dev(torch, r, segs)
    for n in (0, 1, 63, 64, 65, 1027):
        hits = torch.full((n + 3, K, 32), 0xA5, dtype=torch.uint8, device=dev.device)
        counts = torch.full((n + 64,), 0x25A5A5A5, dtype=torch.int32, device=dev.device)
        torch.cuda.synchronize(r.device)
        res = r.trace_all(dev, p, K, hits=hits, counts=counts, nsegs=n)
        r.synchronize()
        assert res[0] is hits and res[1] is counts
        c = counts.cpu().numpy().view(np.uint32)
        h = hits.cpu().numpy()
        assert c[:n].tobytes() == wc[:n].tobytes() and (c[n:] == 0x25A5A5A5).all(), n
        AH.same_records(h[:n].view(T.QHIT).reshape(n, K), wh[:n])
        assert (h[n:] == 0xA5).all(), n
        # counts only: the records are not touched
        hits2 = torch.full((n + 3, K, 32), 0xA5, dtype=torch.uint8, device=dev.device)
        torch.cuda.synchronize(r.device)
        none, c2 = r.trace_all(dev, p, K, want_hits=False, nsegs=n)
        r.synchronize()
        assert none is None and c2.cpu().numpy().view(np.uint32).tobytes() == wc[:n].tobytes(), n
        assert (hits2.cpu().numpy() == 0xA5).all()
        # the host path of the same size, into padded arrays
        hh = np.zeros((n + 3, K), T.QHIT)
        hh.view(np.uint8)[:] = 0xA5
        hc = np.full(n + 64, 0x25A5A5A5, np.uint32)
        r.trace_all(segs[:n], p, K, hits=hh, counts=hc)
        AH.same_records(hh[:n], wh[:n])
        assert hc[:n].tobytes() == wc[:n].tobytes() and (hc[n:] == 0x25A5A5A5).all(), n
        assert (hh[n:].view(np.uint8) == 0xA5).all(), n
    h0, c0 = r.trace_all(None, p, K)  # nsegs == 0 is fine, and launches nothing
    assert h0.shape == (0, K) and c0.shape == (0,)
    # device arrays move as 16-byte vectors and 4-byte words: an offset view is refused on the host
    raw = torch.zeros(32 * 8 + 16, dtype=torch.uint8, device=dev.device)
    off = raw[8:8 + 32 * 8]
    assert off.data_ptr() % 16 == 8
    hits = torch.full((8 * K * 32 + 16,), 0xA5, dtype=torch.uint8, device=dev.device)
    counts = torch.full((8 * 4 + 4,), 0xA5, dtype=torch.uint8, device=dev.device)
    torch.cuda.synchronize(r.device)
    for a_segs, a_hits, a_counts in ((off, hits[:8 * K * 32], counts[:32]), (dev, hits[8:8 + 8 * K * 32], counts[:32]),
                                     (dev, hits[:8 * K * 32], counts[2:34])):
        with pytest.raises(TrtError, match="aligned") as e:
            r.trace_all(a_segs, p, K, hits=a_hits, counts=a_counts, nsegs=8)
        assert e.value.code == T.TRT_ERR_INVALID
    r.synchronize()
    assert (hits.cpu().numpy() == 0xA5).all() and (counts.cpu().numpy() == 0xA5).all()
    for bad_k in (0, 33):
        with pytest.raises(TrtError, match="max_hits") as e:
            r.trace_all(segs[:4], p, bad_k)
        assert e.value.code == T.TRT_ERR_INVALID
    with pytest.raises(TrtError) as e:  # counters are not offered
        r.trace_all(segs, sc.params(flags=sc.flags | T.FLAG_COUNT), K)
    assert e.value.code == T.TRT_ERR_INVALID
    with pytest.raises(TrtError) as e:  # NULL segs
        r.trace_all(None, p, K, nsegs=3)
    assert e.value.code == T.TRT_ERR_INVALID
    with Renderer(r.device) as fresh:
        with pytest.raises(TrtError) as e:
            fresh.trace_all(segs[:4], p, K)
        assert e.value.code == T.TRT_ERR_NOSCENE


def test_query_on_a_torch_stream(use, scenes, refs):
    torch = pytest.importorskip("torch")
    sc = scenes["C3"]
    segs = refs["C3"][0]
    r = use(sc)
    p = sc.params()
    wh, wc = r.trace_all(segs, p, 8)
    dev = to_dev(torch, r, segs)
    s = torch.cuda.Stream(device=r.device)
    r.set_stream(s)
    try:
        with torch.cuda.stream(s):
            hits, counts = r.trace_all(dev, p, 8)
            hits, counts = hits.cpu(), counts.cpu()  # on s, after the query
        s.synchronize()
    finally:
        r.set_stream(None)
    assert hits.numpy().tobytes() == wh.tobytes() and counts.numpy().view(np.uint32).tobytes() == wc.tobytes()
    hits, counts, st = r.trace_all(dev, p, 8, timing=True)
    assert hits.cpu().numpy().tobytes() == wh.tobytes() and st["kernel_ms"] > 0.0


def test_a_query_leaves_frames_and_ray_queries_as_they_were(use, scenes, refs):
    torch = pytest.importorskip("torch")
    rays = random_rays(500, 9)
    for name in ("C2", "C3"):
        sc = scenes[name]
        segs = refs[name][0]
        r = use(sc)
        p = sc.params()

        def state():
            frame, _, _ = r.draw_frame(p)
            _, _, hits, _ = r.trace_rays(rays, p, want8=False, want_hits=True)
            return frame.tobytes(), hits.tobytes(), r.occluded(segs, p).tobytes()

        before = state()
        r.trace_all(segs, p, 8)
        r.trace_all(segs, sc.params(flags=_no_floor(sc) | T.FLAG_BATCH_WALK), 2, want_hits=False)
        r.trace_all(to_dev(torch, r, segs), p, 32)
        r.synchronize()
        assert state() == before, name


# ---- 7: Renderer.contains ---------------------------------------------------------------------------

CENTRE, RADIUS, DIRECTION = np.array((2.5, -2.0, -10.0)), 1.5, (0.3, 1.0, 0.2)


def test_contains_on_the_icosphere(use, scenes):
    sc = scenes["C3"]
    rng = np.random.default_rng(5)
    u = rng.normal(size=(400, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rad = np.concatenate([rng.uniform(0.0, 1.3, 200), rng.uniform(1.6, 3.0, 200)])
    pts = (CENTRE + u * rad[:, None]).astype(f32)
    segs = np.zeros(400, T.QSEG)
    segs["org"], segs["dir"], segs["tmax"] = pts, np.asarray(DIRECTION, f32), T.QSEG_MAX_T
    tot = AH.totals(AH.all_candidates(sc, segs, int(sc.flags) & ~(T.FLAG_FLOOR | T.FLAG_SPHERES)))
    want = tot % 2 == 1
    assert want[:200].all() and not want[200:].any() and tot.max() <= 2, "the reference itself: 200 inside, 200 outside"
    r = use(sc)
    got = r.contains(pts, sc.params())
    assert got.dtype == bool and got.shape == (400,)
    assert np.array_equal(got, want)
    assert np.array_equal(r.contains(pts, sc.params(), direction=DIRECTION), want)
