"""What a frame with RT_HIP_FLAG_BOX_BVH is told on the host, on the CPU: the refusals of the request
(rt_amd/csrc/frame_setup.cpp), its launch plan (rt_amd/csrc/launch_plan.cpp), the flag's refusal by passes (progressive.cpp) and by
rt_headless.  tests/native/box_bvh_plan_dump.cpp is built with g++ alone."""
import shutil
import subprocess

import pytest

from rt_amd import capi
from tests import pass_plan
from tests.conftest import ROOT
from tests.test_box_plan import REFUSED_WITH, fields, request

SOURCES = [str(ROOT / "tests" / "native" / "box_bvh_plan_dump.cpp"), str(ROOT / "rt_amd" / "csrc" / "launch_plan.cpp"), str(ROOT / "rt_amd" / "csrc" / "frame_setup.cpp")]
BOXES = capi.RT_HIP_FLAG_TRACE_BOXES
TREE = capi.RT_HIP_FLAG_BOX_BVH
KERNEL = {name: code for code, name in capi.KERNEL_NAMES.items()}
SCAN_BVH, SCAN_BVH_BOXES, SCAN_BVH_BOXTREE = -4, -8, -9  # launch_plan.hpp
STACKS = 24 * 1024  # bvh_max_depth words for each of a workgroup's 256 lanes

CASES = {
    "257_boxes": request(0, 0, 257, flags=BOXES | TREE, frame=(32, 18), spp=16),
    "100000_boxes": request(0, 0, 100000, flags=BOXES | TREE, frame=(32, 18), spp=16),
    "257_boxes_flagless": request(0, 0, 257, flags=BOXES, frame=(32, 18), spp=16),
    "one_box_two_spheres": request(2, 0, 1, flags=BOXES | TREE),
    "mixed_2000_boxes_1400_spheres": request(1400, 1, 2000, flags=BOXES | TREE, frame=(32, 18), spp=16),
    "sm_table": request(45, 1, 300, flags=BOXES | TREE | capi.RT_HIP_FLAG_SM_MATERIALS),
    "with_bvh_flag": request(200, 0, 300, flags=BOXES | TREE | capi.RT_HIP_FLAG_BVH),
    "with_bvh_device_build": request(200, 0, 300, flags=BOXES | TREE | capi.RT_HIP_FLAG_BVH | capi.RT_HIP_FLAG_BVH_DEVICE_BUILD),
    "tilted_camera": request(2, 1, 300, flags=BOXES | TREE, camera=1),
    "headline_frame_host": request(3, 1, 10000, flags=BOXES | TREE, frame=(1920, 1080), spp=64, host=1),
    "whole_chunks_flag": request(2, 0, 300, flags=BOXES | TREE | capi.RT_HIP_FLAG_FORCE_WHOLE_CHUNKS),
    "lds_too_small": request(2, 0, 300, flags=BOXES | TREE, frame=(1920, 1080), spp=4096),
    "no_box_with_flags": request(2, 0, 0, flags=BOXES | TREE),
    "no_box_flagless": request(2, 0, 0, flags=0),
    "no_box_many_spheres_with_flags": request(1500, 1, 0, flags=BOXES | TREE, frame=(32, 18), spp=16),
    "no_box_many_spheres_flagless": request(1500, 1, 0, flags=0, frame=(32, 18), spp=16),
    "preview_ignores_it": request(2, 1, 300, flags=BOXES | TREE | capi.RT_HIP_FLAG_PREVIEW),
    "preview_ignores_it_alone": request(2, 1, 300, flags=TREE | capi.RT_HIP_FLAG_PREVIEW),
    "without_trace_boxes": request(2, 0, 300, flags=TREE),
    "without_trace_boxes_no_box": request(2, 0, 0, flags=TREE),
    **{f"with_{name}": request(2, 0, 300, flags=BOXES | TREE | bit) for name, bit in REFUSED_WITH.items()},
    **{f"with_{name}_no_box": request(2, 0, 0, flags=BOXES | TREE | bit) for name, bit in REFUSED_WITH.items()},
}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("box_bvh_plan") / "box_bvh_plan_dump"
    built = subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *SOURCES, "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    out = subprocess.run([str(exe)], input="".join(" ".join(str(v) for v in r) + "\n" for r in CASES.values()), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(CASES)
    return dict(zip(CASES, lines))


def test_any_number_of_boxes_is_planned_onto_the_box_tree_build(answers):
    for name in ("257_boxes", "100000_boxes", "one_box_two_spheres", "mixed_2000_boxes_1400_spheres", "sm_table", "with_bvh_flag", "with_bvh_device_build", "tilted_camera", "headline_frame_host", "whole_chunks_flag"):
        plan = fields(answers[name])
        assert (plan["variant"], plan["scan"], plan["build"], plan["boxes"], plan["box_tree"]) == (KERNEL["bvh"], SCAN_BVH, SCAN_BVH_BOXTREE, 1, 1), name
        assert plan["table_bytes"] == STACKS and plan["lds_bytes"] == STACKS + plan["slot_bytes"] <= 64 * 1024, name  # the stacks alone
        assert plan["halves"] == plan["sub_chunk_items"] == plan["big_scene"] == plan["pass"] == plan["planes"] == plan["general_camera"] == 0 and plan["persistent_slot"] == -1, name
    assert fields(answers["sm_table"])["sm_table"] == 1 and fields(answers["257_boxes"])["sm_table"] == 0


def test_without_the_flag_257_boxes_are_refused_with_todays_text(answers):
    assert answers["257_boxes_flagless"] == "refused 5 rt_hip_render_device: RT_HIP_FLAG_TRACE_BOXES: 257 boxes: at most 256 are traced (a linear scan from LDS; there is no hierarchy over boxes)"


def test_without_a_box_the_flag_changes_nothing(answers):
    assert answers["no_box_with_flags"] == answers["no_box_flagless"]
    assert answers["no_box_many_spheres_with_flags"] == answers["no_box_many_spheres_flagless"]
    plain = fields(answers["no_box_flagless"])
    assert plain["variant"] == KERNEL["small"] and plain["boxes"] == plain["box_tree"] == 0
    assert fields(answers["no_box_many_spheres_flagless"])["variant"] == KERNEL["streamed"]
    for name in ("preview_ignores_it", "preview_ignores_it_alone"):
        assert "boxes=0 box_tree=0" in answers[name], name


def test_refusals_name_the_flag(answers):
    for case in ("without_trace_boxes", "without_trace_boxes_no_box"):
        assert answers[case].startswith("refused 5 rt_hip_render_device: RT_HIP_FLAG_BOX_BVH ") and "RT_HIP_FLAG_TRACE_BOXES" in answers[case], answers[case]
    for name in REFUSED_WITH:
        for case in (f"with_{name}", f"with_{name}_no_box"):
            assert answers[case].startswith("refused 5 rt_hip_render_device: RT_HIP_FLAG_BOX_BVH "), answers[case]
    assert "RT_HIP_FLAG_FAST" in answers["with_fast"] and "RT_HIP_FLAG_FORCE_HALF_CHUNKS" in answers["with_force_half_chunks"]
    for name in ("force_tiled", "force_resident", "force_streamed"):
        assert "RT_HIP_FLAG_FORCE_TILED / _RESIDENT / _STREAMED" in answers[f"with_{name}"]
    assert answers["lds_too_small"].startswith("refused 5 rt_hip_render_device: RT_HIP_FLAG_BOX_BVH: ") and "LDS" in answers["lds_too_small"]


def test_passes_refuse_the_flag_by_name():
    if pass_plan.executable() is None:
        pytest.skip("no g++")
    assert pass_plan.refused_flag(BOXES | TREE) == "RT_HIP_FLAG_BOX_BVH"
    assert pass_plan.refused_flag(TREE | capi.RT_HIP_FLAG_SM_MATERIALS) == "RT_HIP_FLAG_BOX_BVH"
    assert pass_plan.refused_flag(BOXES) == "RT_HIP_FLAG_TRACE_BOXES"  # (as before)


def test_headless_refuses_box_bvh_without_boxes():
    binary = ROOT / "rt_amd" / "bin" / "rt_headless"
    run = lambda *args: subprocess.run([str(binary), *args], cwd=ROOT, capture_output=True, text=True, timeout=60)  # noqa: E731
    out = run("--box-bvh", "--renderer", "hip", "--scene", "basic.toml", "--size", "16x8")
    assert out.returncode == 2 and "--box-bvh" in out.stderr and "--boxes" in out.stderr
    out = run("--boxes", "--box-bvh", "--progressive", "16", "--renderer", "hip", "--scene", "basic.toml", "--size", "16x8")
    assert out.returncode == 2 and "--progressive" in out.stderr
    assert run("--list").stdout == run("--list", "--boxes", "--box-bvh").stdout  # the registry's list, unchanged
