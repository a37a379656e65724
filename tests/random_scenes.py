"""Scenes that are not the reference's, shared by tests/test_random_scenes.py (CPU) and
tests/test_gpu_random_scenes.py: everything a frame reads arrives through the caller's UBO (four
spheres with their materials, three lights, the camera) and params.fov, and the fast C2 paths
(sky spans, sphere intervals, shadow occluder masks, floor class, dark-shadow skip) are proofs
computed from those values.  random_ubo(seed) draws all of them; CASES are hand-made UBOs at the
edges a draw rarely lands on.  make_ubo rounds to float32, so the oracle and the kernel read the
same bytes.  No GPU is needed to import this module."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from vkcomputeshader_tinyraytracer_amd import scene as S, types as T

W, H = 72, 52  # partial 8x8 and 16x16 tiles on both axes
ENV = (256, 128)
FLAGS = T.FLAG_SPHERES | T.FLAG_FLOOR | T.FLAG_ENVMAP | T.FLAG_ROW_QUIRK
SEEDS = tuple(range(32))
DEPTHS = (1, 4, 6, 20)  # a seed renders at DEPTHS[seed % 4]
CASE_DEPTHS = (4, 20)
WALK_SPEED = 0.5  # camera_path step of the multi-frame launches: silhouettes cross tiles

# The five material kinds: albedo = (diffuse, specular, reflect, refract) weights uniform in [0, 1],
# with the named weights zeroed.  "black" zeroes all four: every shadow query of such a sphere adds
# nothing, which is the dark-shadow skip on a sphere.
KINDS = {
    "full": (),
    "diffuse_specular_only": (2, 3),
    "reflect_refract_only": (0, 1),
    "no_refraction": (3,),
    "black": (0, 1, 2, 3),
}
# Specular exponents stay >= 1: the kernel's pow is written for y > 0 (include/trt/scene_types.h).
EXPONENTS = (1.0, 2.5, 10.0, 50.0, 125.0, 1425.0)
IORS = (1.0, 1.05, 1.33, 1.5, 2.4, 0.8)
FOVS = (0.5, 1.05, 1.6, 2.4)

# The parity log of the GPU file (TRT_PARITY_LOG, tests/helpers.py) over these scenes.  Every
# comparison of that log is within 1 LSB and within FLOAT_TOL; the cap on the share of pixels that
# differ by that 1 LSB is helpers.MAX_FRAC unless the log shows that these scenes need their own,
# which is then twice the log's worst fraction and never above 0.02 (the rule helpers.py states).
PARITY_LOG = "profiles/random_scenes_parity.jsonl"
MAX_FRAC = None  # None: helpers.MAX_FRAC holds


@dataclass
class Case:
    """One UBO with the frame settings it is rendered under."""

    name: str
    ubo: np.ndarray
    fov: float = 1.05
    width: int = W
    height: int = H
    flags: int = FLAGS

    def scene(self, ubo=None, **kw) -> S.Scene:
        args = dict(width=self.width, height=self.height, max_depth=4, flags=self.flags, env=S.cached_envmap(*ENV))
        args.update(kw)
        return S.Scene(self.name, self.ubo if ubo is None else ubo, **args)

    def params(self, **kw) -> T.Params:
        args = dict(width=self.width, height=self.height, max_depth=4, flags=self.flags, fov=self.fov)
        args.update(kw)
        return T.make_params(**args)

    def cam(self) -> tuple:
        return tuple(float(v) for v in self.ubo["camPos"][:3])

    def with_reference_materials(self) -> np.ndarray:
        """The UBO with the reference's four materials on its geometry: for hit masks taken from
        colour != background, which a black sphere would defeat."""
        u = self.ubo.copy()
        for i, (_, mat) in enumerate(S.SPHERES):
            u[f"sphere{i}"]["material"] = mat
        return u

    def geometry(self):
        """(4 x (centre, radius), 3 x light) as float32 arrays."""
        sph = np.array([self.ubo[f"sphere{i}"]["center_radius"] for i in range(4)], np.float32)
        lts = np.array([self.ubo[f"light{i}"][:3] for i in range(3)], np.float32)
        return sph, lts


def random_material(rng, kind: str) -> np.ndarray:
    albedo = rng.uniform(0.0, 1.0, 4)
    for k in KINDS[kind]:
        albedo[k] = 0.0
    kd = rng.uniform(0.0, 1.0, 3)
    return S.material(tuple(albedo), (*kd, rng.choice(EXPONENTS)), (rng.choice(IORS), 0.0, 0.0, 0.0))


def random_ubo(seed: int) -> Case:
    rng = np.random.default_rng(seed)
    kinds = list(KINDS)
    spheres = []
    for _ in range(4):
        cr = (rng.uniform(-8, 8), rng.uniform(-4.5, 6), rng.uniform(-28, -5), rng.uniform(0.3, 4))
        spheres.append((cr, random_material(rng, kinds[rng.integers(len(kinds))])))
    ang = rng.uniform(0, 2 * np.pi, 3)
    rad = rng.uniform(25, 60, 3)
    lights = np.stack([rad * np.cos(ang), rng.uniform(15, 50, 3), -17 + rad * np.sin(ang)], 1)
    cam = (rng.uniform(-6, 6), rng.uniform(-3.5, 6), rng.uniform(-4, 8))
    fov = float(rng.choice(FOVS))
    flags = FLAGS | (T.FLAG_CHECKER if seed % 3 == 0 else 0)
    return Case(f"seed{seed}", S.make_ubo(cam, tuple(spheres), tuple(map(tuple, lights))), fov=fov, flags=flags)


def seed_depth(seed: int) -> int:
    return DEPTHS[seed % 4]


# ---- hand-made cases --------------------------------------------------------------------------

GLASS_C, GLASS_R = S.SPHERES[1][0][:3], S.SPHERES[1][0][3]
MIRROR_C = S.SPHERES[3][0][:3]


def _mat(base, albedo=None, exponent=None, ior=None):
    m = base.copy()
    if albedo is not None:
        m["albedo"] = albedo
    if exponent is not None:
        m["diffuse_specular"][3] = exponent
    if ior is not None:
        m["refractive"][0] = ior
    return m


def _spheres(**moved):
    """The reference's spheres with sphere<i> = ((centre, radius) or None, material or None)."""
    out = list(S.SPHERES)
    for key, (cr, mat) in moved.items():
        i = int(key[1:])
        out[i] = (out[i][0] if cr is None else cr, out[i][1] if mat is None else mat)
    return tuple(out)


def _lights(**moved):
    out = list(S.LIGHTS)
    for key, pos in moved.items():
        out[int(key[1:])] = pos
    return tuple(out)


def _cases() -> dict:
    glass133 = _mat(S.GLASS, ior=1.33)
    one_way_mirror = S.material((0.1, 0.3, 1.0, 0.0), (0.8, 0.8, 0.9, 50.0), (1.0, 0.0, 0.0, 0.0))
    c = {}

    def add(name, cam=(0.0, 0.0, 0.0), spheres=S.SPHERES, lights=S.LIGHTS, **kw):
        c[name] = Case(name, S.make_ubo(cam, spheres, lights), **kw)

    # cameras
    add("cam_inside_glass", cam=(GLASS_C[0] + 0.5, GLASS_C[1], GLASS_C[2] + 1.0))
    add("cam_inside_mirror", cam=(MIRROR_C[0], MIRROR_C[1] - 1.0, MIRROR_C[2] + 2.0))
    add("cam_just_outside_glass", cam=(GLASS_C[0], GLASS_C[1], GLASS_C[2] + GLASS_R + 1e-3))
    add("cam_below_floor", cam=(0.0, -6.0, 0.0))
    add("cam_on_floor_plane", cam=(0.0, -4.0, 0.0))
    add("cam_far_back", cam=(0.0, 0.0, 1000.0))
    add("fov_narrow", fov=0.3)
    add("fov_wide", fov=2.6)
    add("tiny_frame", cam=(0.5, 0.25, 1.0), width=9, height=7)
    # spheres against the floor plane y = -4
    add("sphere_tangent_to_floor", spheres=_spheres(s0=((-3.0, -2.0, -16.0, 2.0), None)))
    add("sphere_cuts_floor", spheres=_spheres(s1=((-1.0, -4.5, -12.0, 2.0), None)))
    add("sphere_below_floor", spheres=_spheres(s2=((1.5, -8.0, -18.0, 3.0), None)))
    # spheres against each other
    add("overlapping_glass", spheres=_spheres(s0=((0.8, -1.2, -12.5, 2.0), glass133)))
    add("nested_glass", spheres=_spheres(s0=((-0.7, -1.3, -11.8, 0.8), glass133)))
    add("duplicate_spheres_first_wins", spheres=_spheres(s1=(S.SPHERES[0][0], S.RED_RUBBER)))
    add("sphere_behind_camera", spheres=_spheres(s3=((0.0, 1.0, 10.0, 3.0), None)))
    add("enclosing_mirror", spheres=_spheres(s3=((0.0, 0.0, -10.0, 60.0), None)))
    add("facing_mirrors", spheres=_spheres(s0=((-3.0, 0.0, -14.0, 2.5), one_way_mirror),
                                           s1=((3.0, 0.0, -14.0, 2.5), _mat(one_way_mirror, exponent=10.0))))
    # materials
    add("refract_weight_one_ior_one", spheres=_spheres(s1=(None, _mat(S.GLASS, albedo=(0.0, 0.5, 0.1, 1.0), ior=1.0))))
    add("ior_below_one", spheres=_spheres(s1=(None, _mat(S.GLASS, ior=0.8))))
    add("ior_diamond", spheres=_spheres(s1=(None, _mat(S.GLASS, ior=2.4))))
    # a specular weight below every reference material's (0.3 is their least), and a full one
    add("specular_only", spheres=_spheres(s0=(None, _mat(S.IVORY, albedo=(0.0, 0.2, 0.0, 0.0), exponent=1.0)),
                                          s2=(None, _mat(S.RED_RUBBER, albedo=(0.0, 1.0, 0.0, 0.0), exponent=1425.0))))
    add("black_sphere", spheres=_spheres(s2=(None, _mat(S.RED_RUBBER, albedo=(0.0, 0.0, 0.0, 0.0)))))
    add("perfect_mirror", spheres=_spheres(s3=(None, _mat(S.MIRROR, albedo=(0.0, 0.0, 1.0, 0.0)))))
    # lights
    add("light_below_floor", lights=_lights(l0=(-5.0, -10.0, -10.0)))
    add("light_inside_sphere", lights=_lights(l1=(MIRROR_C[0], MIRROR_C[1], MIRROR_C[2] + 1.0)))
    add("light_between_spheres", lights=_lights(l2=(-1.0, 1.5, -15.0)))
    add("coincident_lights", lights=_lights(l1=S.LIGHTS[0]))
    add("light_at_camera", lights=_lights(l0=(0.0, 0.0, 0.0)))
    return c


CASES = _cases()


def all_cases() -> dict:
    """name -> Case of the hand-made cases and the seeds."""
    out = dict(CASES)
    for s in SEEDS:
        k = random_ubo(s)
        out[k.name] = k
    return out
