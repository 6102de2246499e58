"""What a frame with RT_HIP_FLAG_DIRECT_LIGHT is told on the host, on the CPU: the refusals of the request
(rt_amd/csrc/frame_setup.cpp) — by the flag's own name without RT_HIP_FLAG_EMISSION and wherever that flag is refused — its launch plan
(rt_amd/csrc/launch_plan.cpp: planned as a light frame, onto the direct builds when the scene has a sampled light, and as the
RT_HIP_FLAG_EMISSION frame field for field when it has none) and the flag's refusal, by name, by passes (progressive.cpp).
tests/native/direct_plan_dump.cpp is built with g++ alone; every request below must come out as tests/golden/launch_plans_direct.txt says."""
import shutil
import subprocess

import pytest

from rt_amd import capi
from tests import pass_plan
from tests.conftest import GOLDEN, ROOT

SOURCES = [str(ROOT / "tests" / "native" / "direct_plan_dump.cpp"), str(ROOT / "rt_amd" / "csrc" / "launch_plan.cpp"), str(ROOT / "rt_amd" / "csrc" / "frame_setup.cpp"), str(ROOT / "rt_amd" / "csrc" / "lights.cpp")]
GOLDEN_PLANS = GOLDEN / "launch_plans_direct.txt"
EMISSION = capi.RT_HIP_FLAG_EMISSION
ALONE = capi.RT_HIP_FLAG_DIRECT_LIGHT
DIRECT = EMISSION | ALONE
SM = capi.RT_HIP_FLAG_SM_MATERIALS
KERNEL = {name: code for code, name in capi.KERNEL_NAMES.items()}
INVALID_ARGUMENT, UNSUPPORTED = 1, 5

REFUSED_WITH = {
    "fast": capi.RT_HIP_FLAG_FAST,
    "force_tiled": capi.RT_HIP_FLAG_FORCE_TILED,
    "force_resident": capi.RT_HIP_FLAG_FORCE_RESIDENT,
    "force_streamed": capi.RT_HIP_FLAG_FORCE_STREAMED,
    "force_half_chunks": capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS,
    "trace_boxes": capi.RT_HIP_FLAG_TRACE_BOXES,
    "box_bvh": capi.RT_HIP_FLAG_TRACE_BOXES | capi.RT_HIP_FLAG_BOX_BVH,
}
ACCEPTED_WITH = {
    "stats": capi.RT_HIP_FLAG_STATS,
    "persistent_frame": capi.RT_HIP_FLAG_PERSISTENT_FRAME,
    "whole_chunks": capi.RT_HIP_FLAG_FORCE_WHOLE_CHUNKS,
}


def request(spheres, planes, flags=DIRECT, frame=(96, 54), spp=20, camera=0, host=0, table=5, lights=1, materials=5, sampled=1):
    return (spheres, planes, frame[0], frame[1], spp, camera, flags, host, table, lights, materials, sampled)


# name -> request (... table_rows n_lights scene_materials n_sampled_lights)
CASES = {
    "small_scene": request(4, 1),
    "small_scene_sm": request(4, 1, flags=DIRECT | SM),
    "small_scene_emission": request(4, 1, flags=EMISSION),
    "small_scene_emission_sm": request(4, 1, flags=EMISSION | SM),
    "small_scene_no_sampled_light": request(4, 1, sampled=0),
    "small_scene_no_sampled_light_sm": request(4, 1, flags=DIRECT | SM, sampled=0),
    "small_scene_no_light": request(4, 1, lights=0, sampled=0),
    "small_scene_flagless": request(4, 1, flags=0),
    "sampled_lights_without_the_flag": request(4, 1, flags=EMISSION, sampled=3),
    "tilted_camera": request(4, 1, camera=1),
    "tilted_camera_sm": request(4, 1, camera=1, flags=DIRECT | SM),
    "other_camera": request(4, 1, camera=2),
    "scalar_load_scan_40_spheres": request(40, 1, sampled=3),
    "scalar_load_scan_40_spheres_sm": request(40, 1, flags=DIRECT | SM, sampled=3),
    "lds_scan_39_spheres": request(39, 1),
    "bvh_flag_200_spheres": request(200, 1, flags=DIRECT | capi.RT_HIP_FLAG_BVH, sampled=256),
    "bvh_flag_200_spheres_sm": request(200, 1, flags=DIRECT | capi.RT_HIP_FLAG_BVH | SM, sampled=256),
    "bvh_flag_200_spheres_emission": request(200, 1, flags=EMISSION | capi.RT_HIP_FLAG_BVH),
    "bvh_flag_200_spheres_no_sampled_light": request(200, 1, flags=DIRECT | capi.RT_HIP_FLAG_BVH, sampled=0),
    "bvh_device_build": request(200, 1, flags=DIRECT | capi.RT_HIP_FLAG_BVH | capi.RT_HIP_FLAG_BVH_DEVICE_BUILD),
    "hierarchy_1301_primitives": request(1300, 1, frame=(32, 18), spp=16),
    "headline_frame_host": request(4, 1, frame=(1920, 1080), spp=64, host=1),
    "headline_frame_host_emission": request(4, 1, frame=(1920, 1080), spp=64, host=1, flags=EMISSION),
    "headline_frame_host_no_sampled_light": request(4, 1, frame=(1920, 1080), spp=64, host=1, sampled=0),
    "preview_ignores_it": request(4, 1, flags=DIRECT | capi.RT_HIP_FLAG_PREVIEW, table=-1),
    "preview_ignores_it_alone": request(4, 1, flags=ALONE | capi.RT_HIP_FLAG_PREVIEW, table=-1),
    "without_emission": request(4, 1, flags=ALONE),
    "without_emission_sm_bvh": request(4, 1, flags=ALONE | SM | capi.RT_HIP_FLAG_BVH),
    "no_table": request(4, 1, table=-1, lights=0, sampled=0),
    "table_of_another_scene": request(4, 1, table=7, lights=2),
    **{f"with_{name}": request(4, 1, flags=DIRECT | bit) for name, bit in REFUSED_WITH.items()},
    **{f"with_{name}_no_sampled_light": request(4, 1, flags=DIRECT | bit, sampled=0) for name, bit in REFUSED_WITH.items()},
    **{f"with_{name}": request(4, 1, flags=DIRECT | bit) for name, bit in ACCEPTED_WITH.items()},
    **{f"bit_{bit}": request(4, 1, flags=DIRECT | (1 << bit)) for bit in (12, 15, 20, 31)},
}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("direct_plan") / "direct_plan_dump"
    built = subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *SOURCES, "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    out = subprocess.run([str(exe)], input="".join(" ".join(str(v) for v in r) + "\n" for r in CASES.values()), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(CASES)
    return dict(zip(CASES, lines))


def fields(line):
    assert not line.startswith("refused"), line
    return {k: int(v) for k, v in (f.split("=") for f in line.split())}


def test_every_plan_is_the_golden_one(answers):
    text = "".join(f"{name}: {' '.join(str(v) for v in CASES[name])} -> {line}\n" for name, line in answers.items())
    assert text == GOLDEN_PLANS.read_text(), "the plans of frames with direct light moved: if that is meant, write the new table to tests/golden/launch_plans_direct.txt"


def build_of(plan):
    return (plan["variant"], plan["scan"], plan["planes"], plan["general_camera"], plan["sm_table"], plan["lights"], plan["direct"])


def test_the_eight_direct_builds_are_reached_by_the_requests_one_expects(answers):
    resident, bvh = KERNEL["resident"], KERNEL["bvh"]
    want = {
        "small_scene": (resident, 0, 0, 0, 0, 1, 1),
        "small_scene_sm": (resident, 0, 0, 0, 1, 1, 1),
        "tilted_camera": (resident, 0, 0, 1, 0, 1, 1),
        "tilted_camera_sm": (resident, 0, 0, 1, 1, 1, 1),
        "scalar_load_scan_40_spheres": (resident, 0, 1, 0, 0, 1, 1),
        "scalar_load_scan_40_spheres_sm": (resident, 0, 1, 0, 1, 1, 1),
        "bvh_flag_200_spheres": (bvh, -4, 0, 0, 0, 1, 1),
        "bvh_flag_200_spheres_sm": (bvh, -4, 0, 0, 1, 1, 1),
    }
    for name, build in want.items():
        assert build_of(fields(answers[name])) == build, name
    assert len(set(want.values())) == 8
    assert build_of(fields(answers["other_camera"])) == want["tilted_camera"]
    assert build_of(fields(answers["lds_scan_39_spheres"])) == want["small_scene"]
    assert build_of(fields(answers["bvh_device_build"])) == want["bvh_flag_200_spheres"]
    assert build_of(fields(answers["hierarchy_1301_primitives"])) == want["bvh_flag_200_spheres"]
    for name, line in answers.items():
        if not line.startswith("refused") and fields(line)["direct"]:
            plan = fields(line)
            assert plan["lights"] == 1  # a direct build is a light build
            assert plan["halves"] == plan["sub_chunk_items"] == plan["big_scene"] == plan["pass"] == plan["boxes"] == 0 and plan["persistent_slot"] == -1, name
            assert plan["lds_bytes"] == plan["table_bytes"] + plan["slot_bytes"] <= 64 * 1024, name  # (the list is read from memory: no LDS of its own)
    for name in ACCEPTED_WITH:
        assert build_of(fields(answers[f"with_{name}"])) == want["small_scene"], name


def test_a_direct_frame_is_planned_as_the_light_frame_but_for_its_build(answers):
    """field for field: only `direct` tells the two plans apart — kernel_variant, grid, tiles and LDS are the light frame's"""
    for direct, emission in (("small_scene", "small_scene_emission"), ("small_scene_sm", "small_scene_emission_sm"), ("bvh_flag_200_spheres", "bvh_flag_200_spheres_emission"), ("headline_frame_host", "headline_frame_host_emission")):
        a, b = fields(answers[direct]), fields(answers[emission])
        assert a.pop("direct") == 1 and b.pop("direct") == 0 and a == b, direct


def test_without_a_sampled_light_the_plan_is_the_emission_plan(answers):
    """byte for byte: plan_launch looks at n, not at the flag"""
    assert answers["small_scene_no_sampled_light"] == answers["small_scene_emission"] == answers["sampled_lights_without_the_flag"]
    assert answers["small_scene_no_sampled_light_sm"] == answers["small_scene_emission_sm"]
    assert answers["bvh_flag_200_spheres_no_sampled_light"] == answers["bvh_flag_200_spheres_emission"]
    assert answers["headline_frame_host_no_sampled_light"] == answers["headline_frame_host_emission"]
    assert answers["small_scene_no_light"] == answers["small_scene_flagless"]  # (and with no light at all, the flag-less plan)
    assert "lights=0 direct=0" in answers["preview_ignores_it"] and answers["preview_ignores_it"] == answers["preview_ignores_it_alone"]


def test_refusals_name_the_flag(answers):
    for case in ("without_emission", "without_emission_sm_bvh"):
        assert answers[case].startswith(f"refused {UNSUPPORTED} rt_hip_render_device: RT_HIP_FLAG_DIRECT_LIGHT ") and "RT_HIP_FLAG_EMISSION" in answers[case] and "not without it" in answers[case]
    for name in REFUSED_WITH:
        for case in (f"with_{name}", f"with_{name}_no_sampled_light"):
            assert answers[case].startswith(f"refused {UNSUPPORTED} rt_hip_render_device: RT_HIP_FLAG_DIRECT_LIGHT "), answers[case]
    assert "RT_HIP_FLAG_FAST" in answers["with_fast"] and "RT_HIP_FLAG_FORCE_HALF_CHUNKS" in answers["with_force_half_chunks"]
    for name in ("force_tiled", "force_resident", "force_streamed"):
        assert "RT_HIP_FLAG_FORCE_TILED / _RESIDENT / _STREAMED" in answers[f"with_{name}"]
    for name in ("trace_boxes", "box_bvh"):
        assert "RT_HIP_FLAG_TRACE_BOXES / RT_HIP_FLAG_BOX_BVH" in answers[f"with_{name}"]
    assert answers["no_table"].startswith(f"refused {INVALID_ARGUMENT} rt_hip_render_device: RT_HIP_FLAG_EMISSION ") and "rt_hip_set_emission" in answers["no_table"]
    other = answers["table_of_another_scene"]
    assert other.startswith(f"refused {INVALID_ARGUMENT} rt_hip_render_device: RT_HIP_FLAG_EMISSION") and "7 rows" in other and "5 materials" in other
    for bit in (12, 15, 20, 31):
        assert answers[f"bit_{bit}"].startswith(f"refused {UNSUPPORTED} rt_hip_render_device: unknown flag bits"), bit


def test_passes_refuse_the_flag_by_name():
    """progressive and adaptive frames: both go through refused_pass_flag — no longer "unknown flag bits" for bit 17"""
    if pass_plan.executable() is None:
        pytest.skip("no g++")
    assert pass_plan.refused_flag(ALONE) == "RT_HIP_FLAG_DIRECT_LIGHT"
    assert pass_plan.refused_flag(ALONE | SM | capi.RT_HIP_FLAG_BVH) == "RT_HIP_FLAG_DIRECT_LIGHT"
    assert pass_plan.refused_flag(DIRECT) == "RT_HIP_FLAG_EMISSION"  # (the flag it modifies is named first)
    for bit in (12, 15, 20, 31):
        assert pass_plan.refused_flag(1 << bit) == "unknown flag bits"
