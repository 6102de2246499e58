"""The numbers the reference's own source text holds for this path, compared with what this repository's host side and
oracle actually do.

The reference has no tests, golden images or known-answer vectors, so the oracle's parity stays "unpinned"
by reference RESULTS.  What the reference does hold is DATA: the constants of `mg_ray_tracer.cpp`, the loader's defaults and
clamps, the material enum's order, the camera's defaults, the pack multiplier, the two benchmark scene files.  Each of
them was extracted from the source with a regular expression (tools/gen_reference_constants.py) into
tests/golden/reference_constants.json and tests/golden/reference_scenes/; none is hard-coded on this side of the comparison.
"""
import json
import re
from pathlib import Path

import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from rt_amd.scene import column
from tests.conftest import GOLDEN

REF = json.loads((GOLDEN / "reference_constants.json").read_text())


def test_material_type_order_is_the_references_enum():
    names = REF["material_types"]
    assert len(names) == 8
    for index, name in enumerate(names):
        pod = rt_amd.Scene.parse(f"materials = [ {{ type = '{name}' }} ]").describe(8, 8)
        assert column(pod.material_type, 1, np.uint32)[0] == index, name
    # ... and the C ABI's constants carry the same numbers
    header = (Path(rt_amd.__file__).resolve().parent.parent / "include" / "rt_hip.h").read_text()
    for index, name in enumerate(names):
        assert re.search(rf"RT_HIP_MATERIAL_{name.upper()}\s*=\s*{index}\b", header), name


def test_loader_defaults_and_clamps_are_the_references():
    loader = REF["loader"]
    spp_default, bounces_default = loader["samples_per_pixel_default"], loader["max_bounces_default"]
    lo, hi = loader["samples_per_pixel_clamp"]
    pod = rt_amd.Scene.parse("").describe(8, 8)
    assert (pod.samples_per_pixel, pod.max_bounces) == (spp_default, bounces_default)
    pod = rt_amd.Scene.parse(f"samples_per_pixel = {int(hi) + 5}\nmax_bounces = 0").describe(8, 8)
    assert (pod.samples_per_pixel, pod.max_bounces) == (hi, lo)

    # per-type default reflectivity: the switch of scene.cpp:544-556
    table = loader["reflectivity_by_type"]
    fallback = loader["reflectivity_default"]
    assert set(table) == {"metal", "dielectric", "air", "vacuum", "ice", "water"}
    for name in ("lambert", "metal", "dielectric", "air", "vacuum", "water", "ice", "diamond"):
        pod = rt_amd.Scene.parse(f"materials = [ {{ type = '{name}' }} ]").describe(8, 8)
        want = np.float32(table.get(name, fallback))
        assert column(pod.material_reflectivity, 1)[0] == want, name
    # default roughness: 0 for dielectric, else the other constant
    for name, want in (("dielectric", loader["roughness_dielectric"]), ("lambert", loader["roughness_default"]), ("metal", loader["roughness_default"])):
        pod = rt_amd.Scene.parse(f"materials = [ {{ type = '{name}' }} ]").describe(8, 8)
        assert column(pod.material_roughness, 1)[0] == np.float32(want)
    # the material an empty scene gets
    empty = loader["empty_scene_material"]
    pod = rt_amd.Scene.parse("").describe(8, 8)
    assert empty["type"] == "lambert" and column(pod.material_type, 1, np.uint32)[0] == 0
    assert column(pod.material_roughness, 1)[0] == np.float32(empty["roughness"]) and column(pod.material_reflectivity, 1)[0] == np.float32(empty["reflectivity"])

    # default primitives
    pod = rt_amd.Scene.parse("spheres = [ {} ]").describe(8, 8)
    got = [column(p, 1)[0] for p in (pod.sphere_center_x, pod.sphere_center_y, pod.sphere_center_z, pod.sphere_radius)]
    assert got == [np.float32(g) for g in loader["sphere_default"]]
    box = loader["box_default"]
    pod = rt_amd.Scene.parse("boxes = [ {} ]").describe(8, 8)
    got = [column(p, 1)[0] for p in (pod.box_center_x, pod.box_center_y, pod.box_center_z, pod.box_extents_x, pod.box_extents_y, pod.box_extents_z)]
    assert got == [np.float32(box[0]), np.float32(box[1]), np.float32(box[2])] + [np.float32(box[3])] * 3
    pod = rt_amd.Scene.parse("planes = [ {} ]").describe(8, 8)
    assert [column(p, 1)[0] for p in (pod.plane_normal_x, pod.plane_normal_y, pod.plane_normal_z)] == [np.float32(g) for g in loader["plane_normal_default"]]


def test_camera_defaults_are_the_references():
    cam = REF["camera"]
    near, far = cam["near"], cam["far"]
    assert cam["vfov_is_pi_over_four"]
    pos = cam["position"]
    scene_default = REF["loader"]["camera_position_default"]
    assert pos == scene_default
    scene = rt_amd.Scene.parse("")
    width, height = 200, 100
    near_point = scene.screen_to_world(width, height, width / 2, height / 2, 0.0)
    far_point = scene.screen_to_world(width, height, width / 2, height / 2, 1.0)
    # the centre ray starts `near` in front of the default eye and ends `far` in front of it, looking down -Z
    assert np.allclose(near_point, [pos[0], pos[1], pos[2] - near], atol=1e-5)
    assert np.allclose(far_point, [pos[0], pos[1], pos[2] - far], rtol=2e-2)  # (binary32 inverse of a near-0.01 / far-1000 projection: ~1 % at depth 1)
    # vertical field of view pi/4: the top edge's ray makes pi/8 with the axis
    top = scene.screen_to_world(width, height, width / 2, 0.0, 1.0) - np.array(pos, dtype=np.float32)
    assert np.arctan2(top[1], -top[2]) == pytest.approx(np.pi / 8, rel=1e-3)


def test_path_constants_of_mg_ray_tracer_are_the_oracles():
    path = REF["path"]
    min_hit = path["min_hit_dist"]
    sky = path["sky"]
    # sky: lerp(white, sky, 0.5 (y + 1)) at y = +1 is the sky colour itself, at y = -1 white
    assert np.allclose(oracle.sky(1.0), sky, atol=1e-7) and np.allclose(oracle.sky(-1.0), [1, 1, 1])
    # min_hit_dist: a sphere whose near surface is closer than that to the ray's origin is skipped, one beyond it is hit
    mat = [(0, 1, 1, 1, 1, 0.5, 0.5)]
    for gap, expect_hit in ((min_hit * 0.5, False), (min_hit * 2.0, True)):
        pod = rt_amd.scene_from_arrays(spheres=[(0, 0, -(1 + gap), 1, 0)], materials=mat)
        dist, kind, _, _ = oracle.closest_hit(pod, np.array([[0, 0, 0]], np.float32), np.array([[0, 0, -1]], np.float32))
        assert bool(kind[0]) == expect_hit, gap
        if expect_hit:
            assert dist[0] == pytest.approx(gap, rel=1e-3)
    # the pack multiplier of rt::colour -> uint32
    scale = path["pack_multiplier"]
    for v in (0.25, 0.5, 0.999, 1.0):
        assert (oracle.pack(v, v, v) >> 24) == int(np.float32(v) * np.float32(scale))
    # reflect(v, n) = v - 2 dot(v, n) n
    assert path["reflect_is_v_minus_2_dot_v_n_n"]


def test_benchmark_scene_files_say_what_the_references_say():
    tomli = pytest.importorskip("tomli")
    here = Path(rt_amd.__file__).resolve().parent.parent / "scenes"
    for name in ("basic.toml", "dielectric.toml"):
        theirs = tomli.loads((GOLDEN / "reference_scenes" / name).read_text())
        ours = tomli.loads((here / name).read_text())
        for doc in (theirs, ours):  # an empty list says the same as no list
            for key in [k for k, v in doc.items() if v == []]:
                del doc[key]
        assert ours == theirs, name
