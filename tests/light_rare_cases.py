"""Constructed 8 x 8 frames that take the scatter tail's rare branches — and the rare branches of the vertex rule itself — through the sixteen
light builds of render_queue (RT_HIP_FLAG_EMISSION; RT_HIP_FLAG_DIRECT_LIGHT, §3.13), shared by
tests/test_light_rare_branches.py (CPU: the censuses say each case reaches what it claims) and tests/test_gpu_light_rare_branches.py
(GPU: every case through every light build it can be steered to, bit for bit against the CPU).  TEST INFRASTRUCTURE, on top of
tests/rare_cases.py, whose cases, machinery and fixture stay as they are.

EMISSION cases ("lights"): every case of rare_cases.all_cases() plus one INERT LAMP — a small sphere of a new last material far off to
the side, with an emission row > 0, so that the light build is planned.  No ray reaches it: the frame is the oracle's frame of the
original case bit for bit (asserted on the CPU), and the oracle's census of the original case stands.

DIRECT cases ("direct"): a sampled lamp changes the frame, and a lambert vertex's step k shifts every later step of its sample by one,
so these are constructed anew; tests/direct_reference.py's render is the reference and its census (the oracle's events under the direct
loop, the restatement's own events, and the own events of ONE watched sample) the proof:

    re-draw         the lambert big sphere with the fixture's step-3 events: under the flag a sample's steps are jitter, k, u, so the zero
                    word is the first scatter's unit vector — behind a vertex that aimed (lamp behind the camera) and behind one that
                    aimed at nothing (lamp behind the sphere: no visible vertex ever aims)
    zero word k     the fixture's step-2 events: k = (0, 0, 0) is light 0, the octahedral corner u = v = -1 and the fold with sgn
    metal first     a metal first vertex draws no k: the step-2 event is still its re-draw, and mirrored paths reach the lamp
                    (a sampled light behind a vertex that did not sample: throughput * E)
    second scatter  tests/golden/stream_events_direct.json: step 5 over two lambert vertices (jitter, k, u, k, u), step 4 over a metal and a
                    lambert one (jitter, u, k, u)
    approx_zero     rare_cases.approx_case's construction with the unit vector of the step one later, lamp in front of the plane (the
                    target aims, its scatter runs behind the shadow query) and behind it (it never aims)
    zero jitter, the tie, the material extremes   the existing constructions with a sampled lamp
    list edges      256 tiny lamps and a vertex that chooses the last; a sampled lamp met behind a vertex that sampled (worth 0), and
                    behind a mirror that follows such a vertex (worth throughput * E again)

Every scene also has a PADDED variant — the same scene plus 44 inert, far, tiny spheres — that the scalar-load scan takes (it starts at 40
spheres); the CPU asserts that the padding changes no bit.  ORACLE_TEST_NO_RARE_RULES is honoured under the direct loop (render_frame
reads it wherever a census is open), so sensitivity is shown for direct cases too."""
from __future__ import annotations

import functools
import json
from dataclasses import dataclass, field
from typing import Callable

import numpy as np

import rt_amd
from oracle import binding as oracle
from tests import direct_reference as direct_ref
from tests import light_reference as light_ref
from tests import rare_cases as rc
from tests.conftest import GOLDEN

W, H = rc.W, rc.H
LAMBERT, METAL, DIELECTRIC = rc.LAMBERT, rc.METAL, rc.DIELECTRIC
INERT_LAMP = (-40.0, 40.0, 40.0, 0.25)  # far off to the side, as rare_cases.BOX is: no ray of any case reaches it (asserted on the CPU)
PADDING = [(-60.0 - 0.5 * i, 50.0, 60.0, 0.01) for i in range(44)]  # inert, far, tiny: with them a scene has at least 40 spheres
GLOW = (2.0, 1.5, 1.0)
DIRECT_EVENTS = json.loads((GOLDEN / "stream_events_direct.json").read_text())


def direct_events_of(step):
    return [e for e in DIRECT_EVENTS if e["step"] == step]


@dataclass(frozen=True)
class LightCase:
    name: str
    klass: str  # the case class of the coverage table
    flag: str  # "lights": RT_HIP_FLAG_EMISSION alone; "direct": with RT_HIP_FLAG_DIRECT_LIGHT
    arrays: Callable  # () -> (spheres, planes, materials, inverse view projection, max_bounces), lamps and their materials included
    glowing: tuple  # material index -> emission row, as ((index, (r, g, b)), ...)
    seed: int
    spp: int
    expect: Callable  # sm -> {event of either census: ("==" | ">=", count)}
    watch: Callable = lambda sm: {}  # sm -> the same over the own events of the sample (target, sample)
    target: int | None = None
    sample: int = 0
    sensitive: bool = False  # the target's float mean differs in bits when the two rare rules are switched off
    nan_ok: bool = False
    base: rc.Case | None = None  # "lights": the case of tests/rare_cases.py's kind this one is, lamp apart
    tables: tuple = (False, True)
    note: str = field(default="", compare=False)

    def pod(self, padded=False, spp=None):
        spheres, planes, materials, ivp, bounces = self.arrays()
        spheres = list(spheres) + ([(*p, 0) for p in PADDING] if padded else [])
        return rt_amd.scene_from_arrays(spheres or None, list(planes) or None, materials, samples_per_pixel=self.spp if spp is None else spp, max_bounces=bounces, inverse_view_projection=ivp)

    def table(self):
        table = np.zeros((len(self.arrays()[2]), 3), dtype=np.float32)
        for index, rgb in self.glowing:
            table[index] = rgb
        return table

    @property
    def target_xy(self):
        return self.target % W, self.target // W

    @property
    def direct(self):
        return self.flag == "direct"


def arrays_of(pod):
    """(spheres, planes, materials, inverse view projection, max_bounces) of an rt_hip_scene, as scene_from_arrays takes them (binary32
    values pass through exactly)"""
    spheres = [(pod.sphere_center_x[i], pod.sphere_center_y[i], pod.sphere_center_z[i], pod.sphere_radius[i], pod.sphere_material[i]) for i in range(pod.n_spheres)]
    planes = [(pod.plane_normal_x[i], pod.plane_normal_y[i], pod.plane_normal_z[i], pod.plane_d[i], pod.plane_material[i]) for i in range(pod.n_planes)]
    materials = [(pod.material_type[m], *pod.material_albedo[4 * m : 4 * m + 4], pod.material_roughness[m], pod.material_reflectivity[m]) for m in range(pod.n_materials)]
    return spheres, planes, materials, np.array(pod.inverse_view_projection[:], dtype=np.float32).reshape(4, 4), pod.max_bounces


def with_lamps(arrays, lamps):
    """`arrays` plus the lamps (x, y, z, r), all of ONE new last material; returns (arrays, the lamp material's index)"""
    spheres, planes, materials, ivp, bounces = arrays
    lamp_material = len(materials)
    return (list(spheres) + [(*lamp, lamp_material) for lamp in lamps], list(planes), list(materials) + [rc.material(LAMBERT, (0.5, 0.5, 0.5))], ivp, bounces), lamp_material


def form_of(ivp):
    pod = rt_amd.scene_from_arrays([(0.0, 0.0, 0.0, 1.0, 0)], None, [rc.material(LAMBERT)], inverse_view_projection=ivp)
    return oracle.primary_ray(pod, W, H, 0, 0, want_form=True)[2]


TILTED = rc.camera((0, 0, 0), (0.2, -0.15, -1))  # a general camera under which every primary ray still hits the big sphere (asserted on the CPU)


# ---- RT_HIP_FLAG_EMISSION: the existing cases with an inert lamp -----------------------------------------------------------------------------
def emission_case(base):
    def arrays():
        return with_lamps(arrays_of(base.pod()), [INERT_LAMP])[0]

    lamp_material = base.pod().n_materials
    klass = "redraw" if base.name.startswith("redraw") else "approx_zero" if base.name.startswith("approx_zero") else "zero_jitter" if base.name.startswith("zero_jitter") else "tie" if "tie" in base.name else "extremes"
    return LightCase(f"lights_{base.name}", klass, "lights", arrays, ((lamp_material, GLOW),), base.seed, base.spp, base.expect, target=base.target, sample=base.sample, sensitive=base.sensitive, nan_ok=base.nan_ok, base=base,
                     tables=base.tables)


def second_camera_for(ivp, u64):
    """A camera a little further back on the axis u that has the OTHER form of primary ray (pinhole against eye form: which one a matrix
    gets hangs on whether two of its entries round to zero, rt_amd/csrc/frame_setup.cpp) — the first of a fixed list of candidates"""
    wanted = "eye" if form_of(ivp) == "pinhole" else "pinhole"
    candidates = [rc.camera(tuple(map(float, -back * u64)), tuple(map(float, scale * u64 + np.array(nudge)))) for back in (0.0, 0.25, 0.5) for scale in (1.0, 2.0, 3.0) for nudge in ((0, 0, 0), (1e-3, 0, 0), (0, 1e-3, 0), (0, 0, 1e-3))]
    return next(c for c in candidates if form_of(c) == wanted)


def extra_emission_bases():
    """The two classes every build must be reached by get a second camera (rare_cases' own re-draw cameras are pinholes, its approx_zero
    cameras eye forms): a re-draw through the tilted camera, and approx_zero on both sides of the rule's threshold through the other form."""
    first = rc.events_of("redraw_first_scatter")
    bases = [rc.redraw_case("redraw_lambert_tilted", first[0], LAMBERT, ivp=TILTED), rc.redraw_case("redraw_metal_tilted", first[1], METAL, ivp=TILTED)]
    seed, pixel = 7, 27
    for name, offsets, kind in (("exact", (0, 0, 0), "lambert_rule"), ("17_0_0", (17, 0, 0), "lambert_near_zero")):
        like = rc.approx_case(f"approx_zero_{name}_second_camera", seed, pixel, 0, offsets, kind)
        spheres, planes, materials, ivp, bounces = arrays_of(like.pod())
        u, _ = oracle.unit_vector(seed, pixel, 0, 1)
        make = rc.scene(spheres, planes, materials, second_camera_for(ivp, u.astype(np.float64)), bounces)
        bases.append(rc.Case(like.name, make, seed, 1, like.expect, target=pixel, sample=0, sensitive=like.sensitive, spheres=False))
    return bases


# ---- RT_HIP_FLAG_DIRECT_LIGHT ------------------------------------------------------------------------------------------------------------
BEHIND_CAMERA = (1.0, 4.0, 3.0, 1.0)  # on the camera's side of the big sphere and outside the frustum (the camera looks down -z from the origin)
BEHIND_SPHERE = (0.0, 0.0, -15.0, 0.5)  # behind the big sphere: cx < 0 at every visible vertex, nothing ever aims
MIRRORED = (0.0, 0.0, 4.0, 1.5)  # straight behind the camera: where the big sphere's cap mirrors paths to
BESIDE_WALL = (-6.0, 0.0, 1.0, 0.5)  # between cap and wall, off to the -x side (the scatters lean to +x, +y, +z)
WALL = [(0.0, 0.0, -1.0, 2.0, 1)]


def sphere_case(name, klass, event, kind, lamp, expect, watch, planes=(), ivp=rc.FRONT, sensitive=True, note=""):
    materials = [rc.material(kind), rc.material(LAMBERT, (0.7, 0.7, 0.7))]
    arrays, lamp_material = with_lamps((rc.BIG_SPHERE, list(planes), materials, ivp, 6), [lamp])
    return LightCase(name, klass, "direct", lambda: arrays, ((lamp_material, GLOW),), event["seed"], event["sample"] + 1, expect, watch, target=event["pixel"], sample=event["sample"], sensitive=sensitive, note=note)


def direct_redraw_cases():
    first, second = rc.events_of("redraw_first_scatter"), rc.events_of("redraw_second_scatter")
    step4, step5 = direct_events_of(4), direct_events_of(5)
    assert len(first) >= 4 and len(second) >= 4 and len(step4) >= 2 and len(step5) >= 2
    one_redraw = lambda sm: {"redraw": ("==", 1)}
    aimed = lambda sm: {"first_vertex_aimed": ("==", 1)}
    not_aimed = lambda sm: {"first_vertex_not_aimed": ("==", 1)}
    never_aims = lambda sm: {"redraw": ("==", 1), "vertex_aimed": ("==", 0), "vertex_not_aimed": (">=", W * H)}
    k_zero = lambda sm: {"zero_word_k": ("==", 1), "redraw": ("==", 0)}
    k_zero_watched = lambda which: (lambda sm: {"zero_word_k": ("==", 1), which: ("==", 1), "fold_below": ("==", 1)})
    cases = [
        # jitter, k, u: the step-3 word is the first scatter's unit vector
        sphere_case("direct_redraw_behind_aimed_vertex", "redraw", second[0], LAMBERT, BEHIND_CAMERA, one_redraw, aimed),
        sphere_case("direct_redraw_behind_aimed_vertex_sample18", "redraw", second[3], LAMBERT, BEHIND_CAMERA, one_redraw, aimed, note="two chunks per pixel"),
        sphere_case("direct_redraw_behind_aimed_vertex_tilted", "redraw", second[2], LAMBERT, BEHIND_CAMERA, one_redraw, aimed, ivp=TILTED, note="the general-camera LDS scan"),
        sphere_case("direct_redraw_behind_vertex_that_aims_at_nothing", "redraw", second[0], LAMBERT, BEHIND_SPHERE, never_aims, not_aimed),
        sphere_case("direct_redraw_behind_vertex_that_aims_at_nothing_tilted", "redraw", second[1], LAMBERT, BEHIND_SPHERE, never_aims, not_aimed, ivp=TILTED, note="three chunks per pixel"),
        # jitter, k: the step-2 word is k itself — no re-draw anywhere, and nothing for the rare rules to switch
        sphere_case("direct_zero_word_k_aims", "zero_word_k", first[0], LAMBERT, BEHIND_CAMERA, k_zero, k_zero_watched("first_vertex_aimed"), sensitive=False),
        sphere_case("direct_zero_word_k_aims_at_nothing", "zero_word_k", first[2], LAMBERT, BEHIND_SPHERE, k_zero, k_zero_watched("first_vertex_not_aimed"), sensitive=False),
        # a metal first vertex draws no k: the step-2 word is its re-draw, and the mirror shows paths the lamp
        sphere_case("direct_redraw_metal_first_vertex", "metal_first", first[1], METAL, MIRRORED, lambda sm: {"redraw": ("==", 1), "sampled_light_after_other_vertex": (">=", 1), "zero_word_k": ("==", 0)}, lambda sm: {}),
    ]
    # the second scatter: off the wall behind the camera that every first scatter reaches (rare_cases.redraw_cases)
    # (one re-draw and no zero k: the word at step 5 / step 4 is the SECOND scatter's unit vector, the only place left for it)
    two_vertices = lambda sm: {"redraw": ("==", 1), "zero_word_k": ("==", 0), "vertex_aimed": (">=", 1), "vertex_not_aimed": (">=", 1)}
    behind_metal = lambda sm: {"redraw": ("==", 1), "zero_word_k": ("==", 0), "metal_scattered": (">=", 1)}
    for i, e in enumerate(step5[:2]):
        cases.append(sphere_case(f"direct_redraw_second_scatter_two_lambert_{i}", "second_scatter", e, LAMBERT, BESIDE_WALL, two_vertices, lambda sm: {}, planes=WALL, note="jitter, k, u, k, u"))
    for i, e in enumerate(step4[:2]):
        cases.append(sphere_case(f"direct_redraw_second_scatter_metal_lambert_{i}", "second_scatter", e, METAL, BESIDE_WALL, behind_metal, lambda sm: {}, planes=WALL, note="jitter, u, k, u"))
    return cases


def direct_approx_case(name, seed, pixel, sample, offsets, kind, lamp_in_front, extra=False, second_camera=False):
    """rare_cases.approx_case under the flag: the target's steps are (jitter,) k, u, so the plane faces the unit vector of the step ONE
    LATER.  The lamp stands beside the camera's axis behind the camera — in front of the plane, off the frustum: the target aims — or
    behind the plane: nothing aims."""
    step = (1 if sample == 0 else 2) + 1
    u, steps = oracle.unit_vector(seed, pixel, sample, step)
    assert steps == 1
    exact = -u.astype(np.float64) + np.array(offsets, dtype=np.float64) * rc.UNIT
    normal = exact.astype(np.float32)
    assert np.array_equal(normal.astype(np.float64), exact), "the offset normal is not a binary32 vector"
    planes = [(*map(float, normal), 3.0, 0)]
    spheres = []
    u64 = u.astype(np.float64)
    if extra:
        spheres = [(*map(float, -5.0 * u64), 1.0, 1)]
        planes.append((*map(float, u), 8.0, 1))
    side = np.cross(u64, (0.0, 0.0, 1.0))
    side /= np.linalg.norm(side)
    lamp = (*map(float, -2.0 * u64 + 3.0 * side), 0.75) if lamp_in_front else (*map(float, 6.0 * u64), 0.75)
    materials = [rc.material(LAMBERT, (0.9, 0.7, 0.5)), rc.material(METAL, (0.8, 0.8, 0.9), 0.1)]
    # the camera at the origin looks along u; the second camera stands a little further back on the same axis (the target pixel still
    # sees the plane) and is whichever of the candidates has the OTHER form of primary ray
    ivp = rc.camera((0, 0, 0), tuple(map(float, u)))
    if second_camera:
        ivp = second_camera_for(ivp, u64)
    arrays, lamp_material = with_lamps((spheres, planes, materials, ivp, 6), [lamp])
    others = {"lambert_rule", "lambert_near_zero"} - {kind}

    def expect(sm):
        out = {kind: (">=" if extra else "==", 1)} if kind != "lambert_ordinary" else {"lambert_ordinary": (">=", W * H)}
        if not extra:
            out.update({other: ("==", 0) for other in others})
        out.update({"vertex_aimed": (">=", 1)} if lamp_in_front else {"vertex_aimed": ("==", 0)} if not extra else {})
        return out

    watch = lambda sm: {"first_vertex_aimed" if lamp_in_front else "first_vertex_not_aimed": ("==", 1)}
    return LightCase(name, "approx_zero", "direct", lambda: arrays, ((lamp_material, GLOW),), seed, sample + 1, expect, watch, target=pixel, sample=sample, sensitive=kind == "lambert_rule")


APPROX_TABLE = [
    ("exact", (0, 0, 0), "lambert_rule"),
    ("16_16_16", (16, 16, 16), "lambert_rule"),
    ("17_0_0", (17, 0, 0), "lambert_near_zero"),
    ("16_m16_16", (16, -16, 16), "lambert_rule"),
    ("0_m17_0", (0, -17, 0), "lambert_near_zero"),
    ("29_0_0", (29, 0, 0), "lambert_near_zero"),
    ("30_0_0", (30, 0, 0), "lambert_ordinary"),
    ("far", (4096, -4096, 4096), "lambert_ordinary"),
]  # rare_cases.approx_cases' whole offset table


def direct_approx_cases():
    seed, pixel = 7, 27
    cases = []
    for in_front, where in ((True, "lamp_in_front"), (False, "lamp_behind")):
        cases += [direct_approx_case(f"direct_approx_zero_{name}_{where}", seed, pixel, 0, offsets, kind, in_front) for name, offsets, kind in APPROX_TABLE]
        cases.append(direct_approx_case(f"direct_approx_zero_sample17_{where}", seed, pixel, 17, (16, 16, -16), "lambert_rule", in_front))
        cases.append(direct_approx_case(f"direct_approx_zero_with_sphere_and_planes_{where}", seed, pixel, 0, (16, 16, 16), "lambert_rule", in_front, extra=True))
        # the other form of primary ray, on both sides of the rule's threshold
        cases.append(direct_approx_case(f"direct_approx_zero_exact_{where}_second_camera", seed, pixel, 0, (0, 0, 0), "lambert_rule", in_front, second_camera=True))
        cases.append(direct_approx_case(f"direct_approx_zero_17_0_0_{where}_second_camera", seed, pixel, 0, (17, 0, 0), "lambert_near_zero", in_front, second_camera=True))
    return cases


def direct_jitter_cases():
    """The fixture's zero-jitter events on basic.toml with the material of its last sphere made a light."""
    def case_of(event):
        base = rc.case(f"zero_jitter_seed{event['seed']}")
        arrays = arrays_of(base.pod())
        glowing = arrays[0][-1][4]
        return LightCase(f"direct_zero_jitter_seed{event['seed']}", "zero_jitter", "direct", lambda: arrays, ((glowing, GLOW),), base.seed, base.spp, lambda sm: {"zero_jitter": ("==", 1), "vertex_aimed": (">=", 1)},
                         target=base.target, sample=base.sample)

    return [case_of(e) for e in rc.events_of("zero_jitter")]


def direct_tie_case():
    base = rc.tie_case()
    arrays, lamp_material = with_lamps(arrays_of(base.pod()), [(3.0, 3.0, -1.0, 0.5)])
    return LightCase("direct_sphere_plane_tie", "tie", "direct", lambda: arrays, ((lamp_material, GLOW),), base.seed, base.spp, lambda sm: {"sphere_plane_tie": (">=", 1), "vertex_aimed": (">=", 1)}, target=base.target)


def direct_extreme_cases():
    """Every scene of rare_cases.extreme_cases() with a lamp above it: NaN, infinite and negative throughputs reach the direct sum."""
    cases = []
    for base in rc.extreme_cases():
        arrays, lamp_material = with_lamps(arrays_of(base.pod()), [(0.5, 5.0, 1.0, 1.0)])
        cases.append(LightCase(f"direct_{base.name}", "extremes", "direct", (lambda a: lambda: a)(arrays), ((lamp_material, (4.0, 3.0, 2.0)),), base.seed, base.spp, lambda sm: {"vertex_aimed": (">=", 1), "shadow_visible": (">=", 1)}, nan_ok=True))
    return cases


def direct_list_edge_cases():
    # 256 tiny lamps in a 16 x 16 grid above a lambert floor: choose_light gives every index, the last among them
    grid = [(-3.0 + 0.4 * (i % 16), 2.5, -3.0 + 0.4 * (i // 16), 0.05) for i in range(256)]
    floor, lamps_material = with_lamps(([(0.0, 0.5, 0.0, 0.5, 0)], [(0.0, 1.0, 0.0, 0.0, 0)], [rc.material(LAMBERT, (0.8, 0.8, 0.8))], rc.EXTREME_CAMERA, 4), grid)
    last = LightCase("direct_256_lamps_the_last_is_chosen", "list_edges", "direct", lambda: floor, ((lamps_material, (8.0, 8.0, 8.0)),), 31, 4, lambda sm: {"chose_last_of_256": (">=", 1), "vertex_aimed": (">=", 1), "shadow_visible": (">=", 1)})
    # a big lamp low over the floor: scatters off the floor run into the lamp their vertex has just sampled
    low, lamp_material = with_lamps(([(0.0, 0.5, 0.0, 0.5, 0)], [(0.0, 1.0, 0.0, 0.0, 0)], [rc.material(LAMBERT, (0.8, 0.8, 0.8))], rc.EXTREME_CAMERA, 4), [(0.0, 3.0, 0.0, 1.5)])
    worth_nothing = LightCase("direct_sampled_lamp_behind_a_sampling_vertex", "list_edges", "direct", lambda: low, ((lamp_material, GLOW),), 32, 4,
                              lambda sm: {"sampled_light_after_sampling_vertex": (">=", 1), "shadow_visible": (">=", 1), "shadow_occluded": (">=", 1)})
    # a mirror ball on the floor under the lamp: floor -> mirror -> lamp is a sampled light behind a vertex that sampled nothing, on a path
    # whose EARLIER vertex did sample — worth throughput * E, which a `sampled_before` left standing would make 0
    mirror, lamp_material = with_lamps(([(1.5, 1.5, 1.0, 1.5, 1)], [(0.0, 1.0, 0.0, 0.0, 0)], [rc.material(LAMBERT, (0.8, 0.8, 0.8)), rc.material(METAL, (0.9, 0.9, 0.9), 0.0)], rc.EXTREME_CAMERA, 6), [(-1.0, 3.5, 1.0, 1.5)])
    worth_something = LightCase("direct_sampled_lamp_behind_a_mirror_behind_a_sampling_vertex", "list_edges", "direct", lambda: mirror, ((lamp_material, GLOW),), 33, 8,
                                lambda sm: {"sampled_light_after_other_vertex_later": (">=", 1), "sampled_light_after_sampling_vertex": (">=", 1)})
    return [last, worth_nothing, worth_something]


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = [emission_case(base) for base in (*rc.all_cases(), *extra_emission_bases())]
    cases += direct_redraw_cases() + direct_approx_cases() + direct_jitter_cases() + [direct_tie_case()] + direct_extreme_cases() + direct_list_edge_cases()
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def case(name):
    return next(c for c in all_cases() if c.name == name)


CASE_TABLES = [(c.name, sm) for c in all_cases() for sm in c.tables]
CLASSES = ("redraw", "approx_zero", "zero_jitter", "tie", "extremes", "zero_word_k", "metal_first", "second_scatter", "list_edges")


# ---- the CPU's answers: computed once, shared, read-only -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name, sm, padded=False):
    """The restatement's frame of the case — tests.light_reference.render / tests.direct_reference.render by its flag: (rgba, rgb, segments)."""
    c = case(name)
    render = direct_ref.render if c.direct else light_ref.render  # (a "lights" case's frame is also oracle.render's of its base: base_reference)
    rgba, rgb, stats = render(c.pod(padded), W, H, c.table(), seed=c.seed, sm_materials=sm)
    rgba.setflags(write=False), rgb.setflags(write=False)
    return rgba, rgb, stats["segments"]


@functools.lru_cache(maxsize=None)
def census(name, sm, rare_rules=True):
    """direct_ref.render_census of a direct case, its target watched: (rgba, rgb, segments, {event of either census: count}, {own event
    of the watched sample: count} | None)"""
    c = case(name)
    assert c.direct
    rgba, rgb, stats, counts, own, watched = direct_ref.render_census(c.pod(), W, H, c.table(), seed=c.seed, sm_materials=sm, rare_rules=rare_rules, watch=None if c.target is None else (c.target, c.sample))
    assert not set(counts) & set(own)
    rgba.setflags(write=False), rgb.setflags(write=False)
    return rgba, rgb, stats["segments"], {**counts, **own}, watched


@functools.lru_cache(maxsize=None)
def base_reference(name, sm):
    """oracle.render of the lamp-less case a "lights" case stands on: (rgba, rgb, segments)"""
    c = case(name)
    rgba, rgb, stats = oracle.render(c.base.pod(), W, H, seed=c.seed, sm_materials=sm)
    rgba.setflags(write=False), rgb.setflags(write=False)
    return rgba, rgb, stats["segments"]


@functools.lru_cache(maxsize=None)
def base_census(name, sm, rare_rules=True):
    """oracle.render_census of that lamp-less case: (rgb, {event: count})"""
    c = case(name)
    _, rgb, _, counts = oracle.render_census(c.base.pod(), W, H, seed=c.seed, sm_materials=sm, rare_rules=rare_rules)
    return rgb, counts


# ---- which builds a case is steered to ---------------------------------------------------------------------------------------------------
def runs_of(c, sm):
    """[(what, flags, padded)]: the frames of one case under one scatter table — the LDS scan with the case's camera form, the scalar-load
    scan (the padded scene), the hierarchy over the host's tree and over the device builder's.  Each is rendered through both entry points.
    The 256-lamp scene has more than 40 spheres unpadded: it cannot reach an LDS scan, and that run is absent."""
    from tests import light_plan

    flags = (light_plan.DIRECT if c.direct else light_plan.EMISSION) | (light_plan.SM if sm else 0)
    runs = [("scalar-load scan", flags, True), ("hierarchy, host build", flags | light_plan.BVH, False), ("hierarchy, device build", flags | light_plan.BVH | light_plan.DEVICE_BUILD, False)]
    if c.pod().n_spheres < 40:
        runs.insert(0, ("LDS scan", flags, False))
    return runs


def coverage(triples):
    """{flag: {build: set of case classes}} of (flag, build, class) triples, and the assertion of what must be reached: all eight builds
    of each flag by the re-draw and the approx_zero class; by every other class the scalar-load scan, the hierarchy and one LDS scan."""
    from tests import light_plan

    table = {flag: {build: set() for build in builds} for flag, builds in light_plan.BUILDS.items()}
    for flag, build, klass in triples:
        table[flag][build].add(klass)
    for flag, builds in table.items():
        for build, classes in builds.items():
            assert {"redraw", "approx_zero"} <= classes, (flag, build, classes)
        for klass in {k for f, _, k in triples if f == flag}:
            reached = {build for build, classes in builds.items() if klass in classes}
            for table_name in ("mg", "sm"):
                assert {f"{flag} (scalar-load scan, {table_name})", f"{flag} (hierarchy, {table_name})"} <= reached, (flag, klass, reached)
                assert reached & {f"{flag} (LDS scan, pinhole, {table_name})", f"{flag} (LDS scan, general camera, {table_name})"}, (flag, klass, reached)
    return table


def print_coverage(table):
    print("\nflag: build: case classes of tests/light_rare_cases.py that reach it")
    for flag, builds in table.items():
        for build, classes in builds.items():
            print(f"  {build}: {', '.join(sorted(classes))}")
