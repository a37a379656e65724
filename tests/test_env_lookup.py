"""The envmap lookup on the CPU (tests/env_lookup_common.py): the direction set reaches every
texel, every clamped edge, both sides of the seam and both poles on every shape, so the GPU test
over the same rays cannot be vacuous; the CPU oracle agrees with the float64 reference of the
lookup (its measured deviation sets the GPU bar); and every modelled mistake of the kernel's fetch
paths moves some ray of the set by at least 100 times that bar."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import env_lookup_common as E
from tests.helpers import FLOAT_TOL
from tests.query_common import f32, normalize32
from vkcomputeshader_tinyraytracer_amd import lib

SHAPES = pytest.mark.parametrize("shape", E.ENV_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")


@SHAPES
def test_rays_are_valid_and_deterministic(shape):
    W, H = shape
    rays = E.directions(W, H)
    bad = ctypes.c_uint32(0)
    assert lib().trt_check_rays(rays.ctypes.data, len(rays), ctypes.byref(bad)) == 0, rays[bad.value]
    assert not rays["org"].any()
    assert rays.tobytes() == E.directions(W, H).tobytes()
    cls = E.direction_classes(W, H)
    assert cls["centres"] == slice(0, W * H) and list(cls.values())[-1].stop == len(rays)
    want = {"centres": W * H, "corners": (W + 1) * (H + 1), "uniform": E.N_UNIFORM, "seam": len(E.SEAM_Z) * len(E.SEAM_Y),
            "poles": 8, "pole_clamp": 4 * E.N_CLAMP_LENGTHS, "axes": 4}
    if E.REGRESSIONS:
        want["regressions"] = len(E.REGRESSIONS)
    assert {k: s.stop - s.start for k, s in cls.items()} == want
    env = E.envmap(W, H)
    assert env.shape == (H, W, 4) and (env[..., 3] == 255).all() and env.tobytes() == E.envmap(W, H).tobytes()


@SHAPES
def test_coverage(shape):
    W, H = shape
    rays = E.directions(W, H)
    r = E.ref64(E.envmap(W, H), rays)
    xf, yf = r["xf"].astype(int), r["yf"].astype(int)
    assert xf.min() == -1 and xf.max() == W - 1 and yf.min() == -1 and yf.max() == H - 1
    ix0, iy0 = np.clip(xf, 0, W - 1), np.clip(yf, 0, H - 1)
    seen = np.zeros((H, W), bool)
    seen[iy0, ix0] = True
    assert seen.all(), np.argwhere(~seen)
    for ex in (-1, W - 1):  # the four corners of the clamped border
        for ey in (-1, H - 1):
            assert ((xf == ex) & (yf == ey)).any(), (ex, ey)
    cls = E.direction_classes(W, H)
    d = normalize32(rays["dir"])
    plus, minus = E.seam_rays(W, H)
    assert (d[plus, 0] < 0).all() and (d[plus, 2] == 0).all() and not np.signbit(d[plus, 2]).any()
    assert (d[minus, 0] < 0).all() and (d[minus, 2] == 0).all() and np.signbit(d[minus, 2]).all()
    assert (xf[plus] == W - 1).all() and (xf[minus] == -1).all()
    poles = d[cls["poles"]]
    assert (poles[:, 1] == 1).sum() == 4 and (poles[:, 1] == -1).sum() == 4
    zeros = {(bool(np.signbit(p[0])), bool(np.signbit(p[2]))) for p in poles if p[1] == 1 and p[0] == 0 and p[2] == 0}
    assert len(zeros) == 4
    assert (yf[cls["poles"]][:4] == -1).all() and (yf[cls["poles"]][4:] == H - 1).all()
    # the clamp before acos: inputs built to round above 1.  (None does: y * (1 / sqrt(y * y)) stayed
    # <= 1 on 5 million float32 lengths in 0.1..10, so through a query the clamp only ever sees 1.)
    y = d[cls["pole_clamp"], 1]
    assert (y == 1).any() and (y == -1).any() and (np.abs(y) > 1 - 2.0 ** -22).all()


@SHAPES
def test_oracle_matches_ref64(shape):
    W, H = shape
    c = E.shape_case(shape)
    r = c["r64"]
    n = len(c["rays"])
    print(f"{W}x{H}: {n} rays, oracle vs ref64: linear {c['E_lin']:.3g}, gamma'd {c['E_gamma']:.3g}, bar {c['tol']:.3g}")
    assert c["counters"]["misses"] == n and c["counters"]["primary_rays"] == n
    assert 16 * 2.0 ** -24 <= c["tol"] <= FLOAT_TOL and c["tol"] == E.bar(c["E_gamma"])
    # float32 arithmetic over a W-texel row: a few ulp of u times W of one texel step
    assert c["E_lin"] <= 64 * 2.0 ** -24 * max(W, H, 4)
    # cast_ray's miss is the same lookup
    lin = np.clip(c["lin"], 0, 1)
    assert np.array_equal(c["ref32"][:, :3], np.power(lin, f32(2.2)).astype(f32))
    assert (c["ref32"][:, 3] == 1).all() and (c["ref8"][:, 3] == 255).all()
    want8 = np.floor(255.0 * r["gamma"] + 0.5).astype(np.int16)
    assert np.abs(c["ref8"][:, :3].astype(np.int16) - want8).max() <= 1


@SHAPES
def test_seam_is_one_texel_column(shape):
    """The sampler clamps where u jumps from 1 to 0.  With the rows of the map made equal a seam
    ray's colour is one texel's: column W - 1 for z = +0.0 (u = 1, both columns of the footprint
    clamped to W - 1), column 0 for z = -0.0 (u = 0) — to the rounding of the blend's four float32
    products and three sums of values <= 1 (8 * 2^-24), where another column is O(0.1) away."""
    W, H = shape
    env = E.envmap(W, H).copy()
    env[:] = env[0]
    rays = E.directions(W, H)
    plus, minus = E.seam_rays(W, H)
    from oracle import oracle as orc

    d = normalize32(rays["dir"])
    for i in np.concatenate([plus, minus]):
        assert orc.direction_to_uv(d[i])[0] == (1.0 if i in plus else 0.0)
    lin = E.oracle_lookup(env, rays[np.concatenate([plus, minus])]).astype(np.float64)
    t = env[0, :, :3].astype(np.float64) / 255.0
    assert np.abs(lin[:len(plus)] - t[W - 1]).max() <= 8 * 2.0 ** -24
    assert np.abs(lin[len(plus):] - t[0]).max() <= 8 * 2.0 ** -24
    # and byte for byte: 255 times such a value rounds to the texel's own byte
    assert np.array_equal(np.rint(lin[:len(plus)] * 255.0), np.broadcast_to(env[0, W - 1, :3], (len(plus), 3)))
    assert np.array_equal(np.rint(lin[len(plus):] * 255.0), np.broadcast_to(env[0, 0, :3], (len(minus), 3)))
    if W > 1:  # and the two columns are told apart
        assert np.abs(t[W - 1] - t[0]).max() > 0.05


@pytest.mark.parametrize("mutant", E.MUTANTS)
@SHAPES
def test_mutants_are_caught(shape, mutant):
    W, H = shape
    c = E.shape_case(shape)
    m = E.ref64(c["env"], c["rays"], mutant)
    dev = float(np.abs(m["gamma"] - c["r64"]["gamma"]).max())
    if not E.mutant_applies(mutant, W, H):
        # left out explicitly: on this shape the mutant is the lookup itself (one column, or one texel)
        assert dev <= 2.0 ** -50  # float64 rounding of the reordered sum at most
        return
    print(f"{W}x{H} {mutant}: worst deviation {dev:.3g}, bar {c['tol']:.3g}")
    assert dev >= 100 * c["tol"], (dev, c["tol"])
