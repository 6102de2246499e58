"""Constructed frames that reach the scatter tail's rare branches ("rare branches"), shared by tests/test_rare_branches.py (CPU:
the oracle's branch census says each case reaches what it claims, and that the frame depends on it) and tests/test_gpu_rare_branches.py (GPU:
every case through every family of the render kernel, bit for bit against the oracle).  TEST INFRASTRUCTURE.

Nothing here is left to luck.  For a fixed pixel the map from a stream's counter to its step word is a bijection, so the one position at
which a pixel draws the zero word can be computed (tools/find_stream_events.py; its recorded finds are tests/golden/stream_events.json);
and the unit vector a step draws is a pure function of (seed, pixel, sample, step) (oracle.unit_vector), so a plane can be placed whose
normal is that vector's negative to the unit of 2^-24.

    re-draw        a sphere every primary ray hits; the event's step is the sample's first scatter: random_unit_vector draws (0, 0, 0)
                   and draws again (random.hpp:61-62).  Lambert, metal; a dielectric, which under the sm table takes ONE draw and no
                   re-draw (the zero draw reflects); the second scatter, off a wall behind the camera that every first scatter reaches.
    approx_zero    no sphere; ONE plane with normal -u + j * 2^-24 per component, camera at the origin looking along u: the target's
                   normal + u is exactly j * 2^-24 — on either side of `approx_zero` (1e-6 lies between 16 and 17 units) and of the
                   kernels' vote (3.0001e-12 lies between the squares of 29 and 30 units).
    zero jitter    the fixture's entries on basic.toml's spheres: a sample > 0 whose jitter is exactly (0, 0).
    materials      three spheres over a plane, 8 spp: reflectivity, roughness and albedo outside anything a random scene holds —
                   what sends NaN, negative and > 1 means to the pack.
"""
from __future__ import annotations

import functools
import json
from dataclasses import dataclass, field
from typing import Callable

import numpy as np

import rt_amd
from oracle import binding as oracle
from tests.conftest import GOLDEN

W = H = 8
LAMBERT, METAL, DIELECTRIC = 0, 1, 2
UNIT = 2.0**-24
BOX = [(40.0, 40.0, 40.0, 0.25, 0.25, 0.25, 0)]  # one box off to the side: no ray of any case reaches it (asserted on the CPU)

EVENTS = json.loads((GOLDEN / "stream_events.json").read_text())


def events_of(kind):
    return [e for e in EVENTS if e["kind"] == kind]


@dataclass(frozen=True)
class Case:
    name: str
    make: Callable  # (spp, boxes) -> rt_hip_scene
    seed: int
    spp: int
    # sm table -> {census event: ("==" | ">=", count)}: what the oracle's census must say of the frame
    expect: Callable
    target: int | None = None  # the pixel the event happens in
    sample: int = 0  # ... and the sample
    sensitive: bool = False  # the target's float mean differs in bits when the rare rules are switched off
    quiet_seed: int | None = None  # a neighbouring seed under which the frame never re-draws / never draws the zero jitter
    spheres: bool = True  # (RT_HIP_FLAG_BVH is for scenes with spheres)
    nan_ok: bool = False  # NaN pixels agree in place, any payload (the material extremes)
    tables: tuple = (False, True)
    note: str = field(default="", compare=False)

    def pod(self, spp=None, boxes=False):
        return self.make(self.spp if spp is None else spp, boxes)

    @property
    def target_xy(self):
        return self.target % W, self.target // W


def camera(position, direction):
    return rt_amd.Scene.parse("").set_camera(position, direction).describe(W, H).inverse_view_projection[:]


def scene(spheres, planes, materials, ivp, bounces=6):
    def make(spp, boxes=False):
        return rt_amd.scene_from_arrays(spheres or None, planes or None, materials, boxes=BOX if boxes else None, samples_per_pixel=spp, max_bounces=bounces, inverse_view_projection=ivp)

    return make


# ---- re-draws ----------------------------------------------------------------------------------------------------------------------------
FRONT = camera((0, 0, 0), (0, 0, -1))
BIG_SPHERE = [(0.0, 0.0, -5.0, 4.5, 0)]  # seen from the origin it spans 64 degrees either side of the axis: every primary ray hits it


def material(kind, albedo=(0.8, 0.6, 0.4), roughness=0.3, reflectivity=1.0):
    return (kind, *albedo, 1.0, roughness, reflectivity)


def redraw_case(name, event, kind, spheres=BIG_SPHERE, planes=(), ivp=FRONT, bounces=6, note=""):
    def expect(sm):
        if kind == DIELECTRIC and sm:  # one draw, no unit vector: the zero draw is below every reflect probability
            return {"redraw": ("==", 0), "dielectric_reflected": (">=", 1)}
        return {"redraw": ("==", 1)}

    materials = [material(kind, reflectivity=1.5 if kind == DIELECTRIC else 1.0), material(LAMBERT, (0.7, 0.7, 0.7))]
    return Case(name, scene(list(spheres), list(planes), materials, ivp, bounces), event["seed"], event["sample"] + 1, expect, target=event["pixel"], sample=event["sample"], sensitive=True, quiet_seed=event["seed"] + 1, note=note)


def redraw_cases():
    first, second = events_of("redraw_first_scatter"), events_of("redraw_second_scatter")
    assert len(first) >= 4 and len(second) >= 3
    return [
        redraw_case("redraw_lambert", first[0], LAMBERT),
        redraw_case("redraw_metal", first[1], METAL),
        redraw_case("redraw_dielectric", first[3], DIELECTRIC, note="under the sm table: no re-draw"),
        redraw_case("redraw_lambert_sample40", first[2], LAMBERT, note="three chunks per pixel"),
        # the big sphere again and a wall behind the camera: the sphere's visible cap has normal.z >= 0.9, so every first scatter heads
        # for the wall z = 2 and scatters there a second time; from there paths do reach the sky
        # (NOT "inside a closed sphere": a sphere met from inside keeps its outward normal, so lambert's normal + u leaves it and metal's
        # mirrored ray is absorbed — no path scatters twice in there, tests/test_rare_branches.py holds that)
        redraw_case("redraw_second_scatter_wall", second[2], LAMBERT, planes=[(0.0, 0.0, -1.0, 2.0, 1)]),
        redraw_case("redraw_second_scatter_wall_sample4", second[0], LAMBERT, planes=[(0.0, 0.0, -1.0, 2.0, 1)]),
        redraw_case("redraw_second_scatter_wall_metal", second[3], METAL, planes=[(0.0, 0.0, -1.0, 2.0, 1)]),
    ]


# ---- approx_zero -------------------------------------------------------------------------------------------------------------------------
def approx_case(name, seed, pixel, sample, offsets, kind, extra=False):
    """`kind`: the census class the TARGET's lambert scatter falls in — worked out from the offsets alone (normal + u = offsets * 2^-24
    exactly): lambert_rule where every |offset| <= 16, else lambert_near_zero where the squares sum to at most 3.0001e-12, else ordinary."""
    step = 1 if sample == 0 else 2  # sample 0 draws no jitter
    u, steps = oracle.unit_vector(seed, pixel, sample, step)
    assert steps == 1
    exact = -u.astype(np.float64) + np.array(offsets, dtype=np.float64) * UNIT
    normal = exact.astype(np.float32)
    assert np.array_equal(normal.astype(np.float64), exact), "the offset normal is not a binary32 vector"
    planes = [(*map(float, normal), 3.0, 0)]  # n . p + 3 = 0: three units in front of the camera
    spheres = []
    if extra:  # a sphere behind the camera — where the target's replaced scatter (the normal: straight back) goes — and a plane behind that
        spheres = [(*map(float, -5.0 * u.astype(np.float64)), 1.0, 1)]
        planes.append((*map(float, u), 8.0, 1))
    materials = [material(LAMBERT, (0.9, 0.7, 0.5)), material(METAL, (0.8, 0.8, 0.9), 0.1)]
    others = {"lambert_rule", "lambert_near_zero"} - {kind}

    def expect(sm):
        out = {kind: (">=" if extra else "==", 1)} if kind != "lambert_ordinary" else {"lambert_ordinary": (">=", W * H)}
        if not extra:
            out.update({other: ("==", 0) for other in others})
        return out

    return Case(name, scene(spheres, planes, materials, camera((0, 0, 0), tuple(map(float, u)))), seed, sample + 1, expect, target=pixel, sample=sample, sensitive=kind == "lambert_rule", spheres=extra)


def approx_cases():
    seed, pixel = 7, 27
    table = [
        ("exact", (0, 0, 0), "lambert_rule"),
        ("16_16_16", (16, 16, 16), "lambert_rule"),  # 9.54e-7 each; the squares sum to 2.73e-12, under the vote's bound
        ("17_0_0", (17, 0, 0), "lambert_near_zero"),  # the vote fires, the rule does not
        ("16_m16_16", (16, -16, 16), "lambert_rule"),
        ("0_m17_0", (0, -17, 0), "lambert_near_zero"),
        ("29_0_0", (29, 0, 0), "lambert_near_zero"),  # 2.988e-12: the last square under the vote's bound ...
        ("30_0_0", (30, 0, 0), "lambert_ordinary"),  # ... 3.197e-12: the first above it
        ("far", (4096, -4096, 4096), "lambert_ordinary"),
    ]
    cases = [approx_case(f"approx_zero_{name}", seed, pixel, 0, offsets, kind) for name, offsets, kind in table]
    cases.append(approx_case("approx_zero_sample17", seed, pixel, 17, (16, 16, -16), "lambert_rule"))  # two chunks; the second pass of a progressive frame
    cases.append(approx_case("approx_zero_with_sphere_and_planes", seed, pixel, 0, (16, 16, 16), "lambert_rule", extra=True))
    return cases


# ---- zero jitter -------------------------------------------------------------------------------------------------------------------------
def jitter_cases():
    def expect(sm):
        return {"zero_jitter": ("==", 1)}

    def make_for(event):
        def make(spp, boxes=False):
            pod = rt_amd.Scene.named("basic").set_sampling(spp).describe(W, H)
            if boxes:
                pod = rt_amd.scene_from_arrays([(pod.sphere_center_x[i], pod.sphere_center_y[i], pod.sphere_center_z[i], pod.sphere_radius[i], pod.sphere_material[i]) for i in range(pod.n_spheres)], None,
                                               [(pod.material_type[m], *pod.material_albedo[4 * m : 4 * m + 4], pod.material_roughness[m], pod.material_reflectivity[m]) for m in range(pod.n_materials)],
                                               boxes=BOX, samples_per_pixel=spp, max_bounces=pod.max_bounces, inverse_view_projection=pod.inverse_view_projection[:])
            return pod

        return make

    return [Case(f"zero_jitter_seed{e['seed']}", make_for(e), e["seed"], e["sample"] + 1, expect, target=e["pixel"], sample=e["sample"], quiet_seed=e["seed"] + 1) for e in events_of("zero_jitter")]


# ---- material extremes -------------------------------------------------------------------------------------------------------------------
EXTREME_CAMERA = camera((0.0, 1.0, 4.0), (0.0, -0.15, -1.0))
KIND_NAMES = {LAMBERT: "lambert", METAL: "metal", DIELECTRIC: "dielectric"}


def extreme_case(name, varied, ground=(0.8, 0.8, 0.3)):
    materials = [material(LAMBERT, ground), varied, material(METAL, (0.9, 0.6, 0.4), 0.2), material(DIELECTRIC, (0.9, 0.95, 1.0), 0.0, 1.5)]
    spheres = [(0.0, 1.0, 0.0, 1.0, 1), (-2.1, 0.8, -0.5, 0.8, 2), (2.0, 0.7, 0.3, 0.7, 3)]
    return Case(name, scene(spheres, [(0.0, 1.0, 0.0, 0.0, 0)], materials, EXTREME_CAMERA, bounces=8), 77, 8, lambda sm: {}, nan_ok=True)


def extreme_cases():
    cases = []
    for kind, kind_name in KIND_NAMES.items():
        for value in (0.0, 1.0, -0.5, 1e30):
            cases.append(extreme_case(f"{kind_name}_reflectivity_{value:g}", material(kind, reflectivity=value)))
        for value in (0.0, -0.25, 1e30):
            cases.append(extreme_case(f"{kind_name}_albedo_{value:g}", material(kind, albedo=(value, value, value), reflectivity=1.5 if kind == DIELECTRIC else 1.0)))
    for value in (0.0, 1.0, 5.0):
        cases.append(extreme_case(f"metal_roughness_{value:g}", material(METAL, roughness=value)))
    # an infinite attenuation (1e30 * 1e30) meets an albedo of 0 on the ground: inf * 0, NaN means
    cases.append(extreme_case("lambert_infinite_attenuation_over_ground_albedo_0", material(LAMBERT, albedo=(1e30, 1e30, 1e30), reflectivity=1e30), ground=(0.0, 0.0, 0.0)))
    return cases


# ---- sphere and plane at equal distance --------------------------------------------------------------------------------------------------
def tie_case():
    """select(spheres, planes) at EQUAL distance (mg_ray_tracer.cpp:96-102: the sphere wins).  The frame's matrix is the front camera's with
    the frame shifted by half a pixel, so that pixel (3, 3)'s sample 0 runs down the axis (direction (1e-8, -1e-8, -1)) from z = -0.01;
    the plane z = -4 answers 3.99 and so does a sphere at z = -5 whose radius is 1 - 11 * 2^-24 (found by stepping the radius by units
    until oracle.closest_hit gave the plane's distance; the census holds it).  One sample: the pixel is the sphere's red or the plane's green."""
    shift = np.eye(4)
    shift[0, 3], shift[1, 3] = 0.125, -0.125  # ndc of the centre of pixel (3, 3) of 8 x 8: (-0.125, 0.125)
    ivp = (np.array(FRONT, dtype=np.float64).reshape(4, 4) @ shift).astype(np.float32)
    materials = [material(LAMBERT, (1.0, 0.0, 0.0)), material(LAMBERT, (0.0, 1.0, 0.0))]
    return Case("sphere_plane_tie", scene([(0.0, 0.0, -5.0, 1.0 - 11 * UNIT, 0)], [(0.0, 0.0, 1.0, 4.0, 1)], materials, ivp, bounces=4), 5, 1, lambda sm: {"sphere_plane_tie": ("==", 1)}, target=3 * W + 3)


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = redraw_cases() + approx_cases() + jitter_cases() + [tie_case()] + extreme_cases()
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def case(name):
    return next(c for c in all_cases() if c.name == name)


CASE_TABLES = [(c.name, sm) for c in all_cases() for sm in c.tables]


# ---- the oracle's answers: computed once, shared, read-only -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name, sm, spp=None):
    """oracle.render of the case at `spp` samples per pixel (None: the case's own): (rgba, rgb, segments)."""
    c = case(name)
    rgba, rgb, stats = oracle.render(c.pod(spp), W, H, seed=c.seed, sm_materials=sm)
    rgba.setflags(write=False), rgb.setflags(write=False)
    return rgba, rgb, stats["segments"]


@functools.lru_cache(maxsize=None)
def census(name, sm, seed=None, rare_rules=True):
    """oracle.render_census of the case (seed None: the case's own): (rgba, rgb, segments, {event: count})."""
    c = case(name)
    rgba, rgb, stats, counts = oracle.render_census(c.pod(), W, H, seed=c.seed if seed is None else seed, sm_materials=sm, rare_rules=rare_rules)
    rgba.setflags(write=False), rgb.setflags(write=False)
    return rgba, rgb, stats["segments"], counts


def same_bits(a, b, nan_ok=False):
    """float arrays equal as uint32; nan_ok: a NaN matches a NaN of any payload, in place."""
    same = a.view(np.uint32) == b.view(np.uint32)
    if nan_ok:
        same |= np.isnan(a) & np.isnan(b)
    return bool(same.all())
