"""What a frame with RT_HIP_FLAG_TRACE_BOXES is told on the host, on the CPU: the refusals of the request
(rt_amd/csrc/frame_setup.cpp), its launch plan (rt_amd/csrc/launch_plan.cpp), the flag's refusal by passes (progressive.cpp) and by
rt_headless.  tests/native/box_plan_dump.cpp is built with g++ alone; every request below must come out as
tests/golden/launch_plans_boxes.txt says."""
import shutil
import subprocess

import pytest

from rt_amd import capi
from tests import pass_plan
from tests.conftest import GOLDEN, ROOT

SOURCES = [str(ROOT / "tests" / "native" / "box_plan_dump.cpp"), str(ROOT / "rt_amd" / "csrc" / "launch_plan.cpp"), str(ROOT / "rt_amd" / "csrc" / "frame_setup.cpp")]
GOLDEN_PLANS = GOLDEN / "launch_plans_boxes.txt"
BOXES = capi.RT_HIP_FLAG_TRACE_BOXES
KERNEL = {name: code for code, name in capi.KERNEL_NAMES.items()}
SCAN_RESIDENT_BOXES, SCAN_BVH_BOXES = -7, -8  # launch_plan.hpp

REFUSED_WITH = {
    "fast": capi.RT_HIP_FLAG_FAST,
    "force_tiled": capi.RT_HIP_FLAG_FORCE_TILED,
    "force_resident": capi.RT_HIP_FLAG_FORCE_RESIDENT,
    "force_streamed": capi.RT_HIP_FLAG_FORCE_STREAMED,
    "force_half_chunks": capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS,
}


def request(spheres, planes, boxes, flags=BOXES, frame=(96, 54), spp=20, camera=0, host=0):
    return (spheres, planes, boxes, frame[0], frame[1], spp, camera, flags, host)


# name -> request (n_spheres n_planes n_boxes width local_rows samples_per_pixel camera flags host_frame)
CASES = {
    "one_box_two_spheres": request(2, 0, 1),
    "one_box_two_spheres_flagless": request(2, 0, 1, flags=0),
    "no_box_with_flag": request(2, 0, 0),
    "no_box_flagless": request(2, 0, 0, flags=0),
    "boxes_only": request(0, 0, 3),
    "tilted_camera": request(2, 1, 3, camera=1),
    "other_camera": request(2, 1, 3, camera=2),
    "sm_table": request(2, 1, 3, flags=BOXES | capi.RT_HIP_FLAG_SM_MATERIALS),
    "scalar_load_scan_45_spheres": request(45, 1, 5),
    "hierarchy_1500_spheres": request(1500, 0, 2, frame=(32, 18), spp=16),
    "bvh_flag_200_spheres": request(200, 0, 7, flags=BOXES | capi.RT_HIP_FLAG_BVH),
    "bvh_device_build": request(200, 0, 7, flags=BOXES | capi.RT_HIP_FLAG_BVH | capi.RT_HIP_FLAG_BVH_DEVICE_BUILD),
    "whole_chunks_flag": request(2, 0, 1, flags=BOXES | capi.RT_HIP_FLAG_FORCE_WHOLE_CHUNKS),
    "headline_frame_host": request(3, 1, 3, frame=(1920, 1080), spp=64, host=1),
    "preview_ignores_it": request(2, 1, 3, flags=BOXES | capi.RT_HIP_FLAG_PREVIEW),
    "256_boxes": request(0, 0, 256, frame=(32, 18), spp=16),
    "257_boxes": request(0, 0, 257, frame=(32, 18), spp=16),
    "lds_too_small": request(0, 1024, 256, frame=(1920, 1080), spp=4096),
    **{f"with_{name}": request(2, 0, 1, flags=BOXES | bit) for name, bit in REFUSED_WITH.items()},
    **{f"with_{name}_no_box": request(2, 0, 0, flags=BOXES | bit) for name, bit in REFUSED_WITH.items()},
}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("box_plan") / "box_plan_dump"
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
    assert text == GOLDEN_PLANS.read_text(), "the plans of frames with traced boxes moved: if that is meant, write the new table to tests/golden/launch_plans_boxes.txt"


def test_the_box_builds_are_the_tile_per_wave_whole_chunk_kernels(answers):
    one = fields(answers["one_box_two_spheres"])
    assert (one["variant"], one["scan"], one["planes"], one["general_camera"], one["boxes"]) == (KERNEL["resident"], 0, 0, 0, 1)  # (not the scalar-register kernel the flagless frame takes)
    assert fields(answers["one_box_two_spheres_flagless"])["variant"] == KERNEL["small"] and fields(answers["one_box_two_spheres_flagless"])["boxes"] == 0
    assert one["table_bytes"] == (2 + 2 * 1) * 16 and one["lds_bytes"] == one["table_bytes"] + one["slot_bytes"]
    assert fields(answers["tilted_camera"])["general_camera"] == 1 and fields(answers["other_camera"])["general_camera"] == 1
    scalar = fields(answers["scalar_load_scan_45_spheres"])
    assert (scalar["variant"], scalar["scan"], scalar["planes"], scalar["boxes"]) == (KERNEL["resident"], 0, 1, 1) and scalar["table_bytes"] == (1 + 2 * 5) * 16
    for name in ("hierarchy_1500_spheres", "bvh_flag_200_spheres", "bvh_device_build"):
        tree = fields(answers[name])
        assert (tree["variant"], tree["scan"], tree["boxes"]) == (KERNEL["bvh"], -4, 1), name
        assert tree["table_bytes"] == 24 * 1024 + 2 * CASES[name][2] * 16, name
    for name, line in answers.items():
        if not line.startswith("refused") and fields(line)["boxes"]:
            plan = fields(line)
            assert plan["halves"] == plan["sub_chunk_items"] == plan["big_scene"] == plan["pass"] == 0 and plan["persistent_slot"] == -1, name
            assert plan["lds_bytes"] <= 64 * 1024, name
    assert fields(answers["256_boxes"])["table_bytes"] == 8192


def test_without_a_box_the_flag_changes_nothing(answers):
    assert answers["no_box_with_flag"] == answers["no_box_flagless"]
    assert fields(answers["no_box_with_flag"])["variant"] == KERNEL["small"]
    assert "boxes=0" in answers["preview_ignores_it"]


def test_refusals_name_the_flag(answers):
    for name in REFUSED_WITH:
        for case in (f"with_{name}", f"with_{name}_no_box"):
            assert answers[case].startswith(f"refused 5 rt_hip_render_device: RT_HIP_FLAG_TRACE_BOXES "), answers[case]
    assert "RT_HIP_FLAG_FAST" in answers["with_fast"] and "RT_HIP_FLAG_FORCE_HALF_CHUNKS" in answers["with_force_half_chunks"]
    for name in ("force_tiled", "force_resident", "force_streamed"):
        assert "RT_HIP_FLAG_FORCE_TILED / _RESIDENT / _STREAMED" in answers[f"with_{name}"]
    assert answers["257_boxes"].startswith("refused 5 rt_hip_render_device: RT_HIP_FLAG_TRACE_BOXES: 257 boxes")
    assert answers["lds_too_small"].startswith("refused 5 rt_hip_render_device: RT_HIP_FLAG_TRACE_BOXES: ") and "LDS" in answers["lds_too_small"]


def test_passes_refuse_the_flag_by_name():
    if pass_plan.executable() is None:
        pytest.skip("no g++")
    assert pass_plan.refused_flag(BOXES) == "RT_HIP_FLAG_TRACE_BOXES"
    assert pass_plan.refused_flag(BOXES | capi.RT_HIP_FLAG_SM_MATERIALS) == "RT_HIP_FLAG_TRACE_BOXES"


def test_headless_refuses_boxes_for_other_renderers_and_passes():
    binary = ROOT / "rt_amd" / "bin" / "rt_headless"
    run = lambda *args: subprocess.run([str(binary), *args], cwd=ROOT, capture_output=True, text=True, timeout=60)  # noqa: E731
    out = run("--boxes", "--renderer", "null", "--scene", "basic.toml", "--size", "16x8")
    assert out.returncode == 2 and "--boxes" in out.stderr and "null_renderer" in out.stderr
    out = run("--boxes", "--progressive", "16", "--renderer", "hip", "--scene", "basic.toml", "--size", "16x8")
    assert out.returncode == 2 and "--boxes" in out.stderr and "--progressive" in out.stderr
    assert run("--list").stdout == run("--list", "--boxes").stdout  # the registry's list, unchanged
