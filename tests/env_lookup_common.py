"""Shared by tests/test_env_lookup.py and tests/test_gpu_env_lookup.py: the envmap lookup
(direction_to_uv + bilinear clamp-to-edge sampling of an RGBA8 image, shader.comp:410-416 and
455-458) as its own operation.  Envmap shapes and contents, a direction set that reaches the seam,
the poles, every clamped edge and every texel, a float64 numpy reference of the lookup, small
variants of that reference that model the mistakes the kernel's three fetch paths invite, and the
CPU oracle's measured deviation from the reference, from which the GPU bar is derived.  No GPU; the
oracle is imported only by the functions that run it."""
from __future__ import annotations

import functools

import numpy as np

from tests.helpers import FLOAT_TOL
from tests.query_common import normalize32
from vkcomputeshader_tinyraytracer_amd import scene as S, types as T

f32, f64 = np.float32, np.float64

# (W, H): widths and heights of 1, 2 and 3, odd row strides (W + 3 even and odd), a width past
# one 256-thread block of envp_kernel, and one even 2:1 control
ENV_SHAPES = ((1, 1), (1, 5), (5, 1), (2, 2), (3, 2), (2, 3), (7, 5), (67, 33), (255, 3), (257, 2), (64, 32))
SEED = 20
N_UNIFORM = 2000
N_CLAMP_LENGTHS = 33  # each as k and (1 + 2^-23) k, up and down

PI_F = float(f32(3.14159265358979323846))  # shader.comp:82 as the float32 the shader holds
GAMMA_F = float(f32(2.2))  # shader.comp:81

SEAM_Z = (0.0, -0.0, 1e-30, -1e-30, 1e-7, -1e-7)
SEAM_Y = (0.0, 0.5, -0.5)

# Rays that once exposed a bug in the lookup, by name: (dx, dy, dz).  None has been found so far.
REGRESSIONS: dict = {}


def envmap(W: int, H: int, seed: int = SEED) -> np.ndarray:
    """(H, W, 4) uint8: seeded uniform random bytes per colour channel, alpha 255.  Neighbouring
    texels differ by O(100) of 255, so a wrong texel or weight is an O(0.1) error."""
    rng = np.random.default_rng([seed, W, H])
    env = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    env[..., 3] = 255
    return env


def env_scene(env: np.ndarray, width: int = 72, height: int = 40, flags: int = T.FLAG_ENVMAP, max_depth: int = 4) -> S.Scene:
    """A scene of nothing but the envmap (every ray a miss) unless `flags` adds to it."""
    return S.Scene("ENV", S.make_ubo(), env=env, width=width, height=height, max_depth=max_depth, flags=flags)


def _classes(W: int, H: int, seed: int):
    """name -> (n, 3) float64 directions, in the order of `directions`."""
    rng = np.random.default_rng([seed, W, H, 1])
    out = {}
    out["centres"] = S.equirect_qrays(W, H)["dir"].reshape(-1, 3).astype(f64)
    u = np.arange(W + 1, dtype=f64) / W
    v = np.arange(H + 1, dtype=f64) / H
    theta = (u * 2.0 * np.pi - np.pi)[None, :]
    phi = (v * np.pi)[:, None]
    out["corners"] = np.stack([np.sin(phi) * np.cos(theta), np.cos(phi) * np.ones_like(theta),
                               np.sin(phi) * np.sin(theta)], -1).reshape(-1, 3)
    d = rng.normal(size=(N_UNIFORM, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out["uniform"] = d * rng.uniform(0.1, 10.0, size=(N_UNIFORM, 1))
    out["seam"] = np.array([(-1.0, y, z) for z in SEAM_Z for y in SEAM_Y], f64)
    zeros = [(x, z) for x in (0.0, -0.0) for z in (0.0, -0.0)]
    out["poles"] = np.array([(x, s, z) for s in (1.0, -1.0) for x, z in zeros], f64)
    # lengths at which y * (1 / sqrt(y * y)) can round to 1 + 2^-23: the clamp before acos
    k = np.concatenate([rng.uniform(0.1, 10.0, size=N_CLAMP_LENGTHS - 3), [1.0, 0.1, 10.0]])
    up = (1.0 + 2.0 ** -23) * k
    out["pole_clamp"] = np.array([(0.0, s * y, 0.0) for y in np.concatenate([up, k]) for s in (1.0, -1.0)], f64)
    out["axes"] = np.array([(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)], f64)
    if REGRESSIONS:
        out["regressions"] = np.array(list(REGRESSIONS.values()), f64)
    return out


def direction_classes(W: int, H: int, seed: int = SEED) -> dict:
    """name -> slice into directions(W, H, seed)."""
    at, out = 0, {}
    for k, d in _classes(W, H, seed).items():
        out[k] = slice(at, at + len(d))
        at += len(d)
    return out


def directions(W: int, H: int, seed: int = SEED) -> np.ndarray:
    """T.QRAY records from the origin: texel centres, texel corners, uniform directions of lengths
    0.1..10, the seam, the poles, the axes and the named regression rays; float64, rounded once."""
    d = np.concatenate(list(_classes(W, H, seed).values()))
    q = np.zeros(len(d), T.QRAY)
    q["dir"] = d.astype(f32)  # keeps the sign of a zero
    return q


def seam_rays(W: int, H: int, seed: int = SEED):
    """Indices into directions() of the seam rays with z = +0.0 and with z = -0.0."""
    s = direction_classes(W, H, seed)["seam"]
    n = len(SEAM_Y)
    return np.arange(s.start, s.start + n), np.arange(s.start + n, s.start + 2 * n)


# ---- the float64 reference and its mutants ----------------------------------------------------

MUTANTS = ("swap_c01_c10", "swap_a_b", "ix1_wraps", "shift_left", "iy1_unclamped", "seam_wraps")


def mutant_applies(name: str, W: int, H: int) -> bool:
    """Whether the mutant computes anything else than ref64 on a W x H map: the transposing ones
    need a second texel in either direction, the column ones a second column."""
    return (W > 1 or H > 1) if name in ("swap_c01_c10", "swap_a_b") else W > 1


def ref64(env: np.ndarray, rays: np.ndarray, mutant: str | None = None) -> dict:
    """The lookup in float64 from the shader's float32 normalize of each direction, with the
    shader's float32 constants widened.  Returns linear and gamma'd (n, 3) RGB and the per-ray
    xf, yf (floor of the texel coordinate before any clamp).  `mutant` selects one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    H, W = env.shape[:2]
    d = normalize32(rays["dir"]).astype(f64)
    theta = np.arctan2(d[:, 2], d[:, 0])
    phi = np.arccos(np.clip(d[:, 1], -1.0, 1.0))
    u = (theta + PI_F) / (2.0 * PI_F)
    v = phi / PI_F
    x, y = u * W - 0.5, v * H - 0.5
    xf, yf = np.floor(x), np.floor(y)
    a, b = x - xf, y - yf
    ix, iy = xf.astype(np.int64), yf.astype(np.int64)
    if mutant == "shift_left":  # a pair-row stride of W + 2 where it is W + 3
        ix = ix - 1
    ix0, ix1 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1)
    iy0, iy1 = np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
    if mutant == "ix1_wraps":
        ix1 = np.where(ix + 1 > W - 1, 0, ix1)
    if mutant == "seam_wraps":  # REPEAT addressing in u: u = 1 is u = 0
        ix0, ix1 = np.mod(ix, W), np.mod(ix + 1, W)
    t = env[..., :3].astype(f64) / 255.0
    c00, c10, c01, c11 = t[iy0, ix0], t[iy0, ix1], t[iy1, ix0], t[iy1, ix1]
    if mutant == "iy1_unclamped":  # row H of column x is row H - 1 of the column after it
        past = (iy + 1 > H - 1)[:, None]
        c01 = np.where(past, t[H - 1, np.mod(ix0 + 1, W)], c01)
        c11 = np.where(past, t[H - 1, np.mod(ix1 + 1, W)], c11)
    if mutant == "swap_c01_c10":
        c01, c10 = c10, c01
    if mutant == "swap_a_b":
        a, b = b, a
    a, b = a[:, None], b[:, None]
    lin = (1 - a) * (1 - b) * c00 + a * (1 - b) * c10 + (1 - a) * b * c01 + a * b * c11
    gamma = np.power(np.clip(lin, 0.0, 1.0), GAMMA_F)
    return {"lin": lin, "gamma": gamma, "xf": xf, "yf": yf}


# ---- the oracle against the reference ---------------------------------------------------------


def oracle_lookup(env: np.ndarray, rays: np.ndarray) -> np.ndarray:
    """The oracle's direction_to_uv + sample_env per ray, on the float32-normalized direction:
    linear (n, 3) float32."""
    from oracle import oracle as orc

    d = normalize32(rays["dir"])
    return np.array([orc.sample_env(env, orc.direction_to_uv(d[i])) for i in range(len(d))], f32).reshape(-1, 3)


def measure(env: np.ndarray, rays: np.ndarray) -> dict:
    """The oracle on `env` along `rays` and its deviation from ref64: its cast_ray colours
    (ref8, ref32, counters, as tests.query_common.oracle_colours), its linear lookup, E_lin and
    E_gamma (the worst absolute deviation of either from ref64) and the bar `tol` they set."""
    from oracle import oracle as orc
    from tests.query_common import oracle_colours

    sc = env_scene(env)
    ref8, ref32, tot = oracle_colours(orc._Bound(sc), sc.params(), rays)
    r = ref64(env, rays)
    lin = oracle_lookup(env, rays)
    e_lin = float(np.abs(lin.astype(f64) - r["lin"]).max())
    e_gamma = float(np.abs(ref32[:, :3].astype(f64) - r["gamma"]).max())
    return {"ref8": ref8, "ref32": ref32, "counters": tot, "lin": lin, "r64": r, "E_lin": e_lin, "E_gamma": e_gamma,
            "tol": bar(e_gamma)}


def bar(e_gamma: float, factor: float = 4.0) -> float:
    """The GPU bar on the gamma'd float output: `factor` times the oracle's own worst deviation
    from ref64 (the kernel multiplies by rounded reciprocals where the oracle divides and calls
    ocml's atan2f / acosf / powf where the oracle calls libm's, so its u, v error can be a small
    multiple of the host's), no less than 16 ulp of 1 (OpenCL's bound for powf at values <= 1) and
    never more than the suite's FLOAT_TOL."""
    return min(FLOAT_TOL, max(factor * e_gamma, 16 * 2.0 ** -24))


@functools.lru_cache(maxsize=None)
def shape_case(shape: tuple, seed: int = SEED) -> dict:
    """Envmap, rays and `measure` of one ENV_SHAPES entry, computed once per process."""
    W, H = shape
    env, rays = envmap(W, H, seed), directions(W, H, seed)
    for a in (env, rays):
        a.setflags(write=False)
    return dict(measure(env, rays), env=env, rays=rays)


def tol(shape: tuple, seed: int = SEED) -> float:
    return shape_case(shape, seed)["tol"]
