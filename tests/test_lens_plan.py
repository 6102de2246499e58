"""What a frame with RT_HIP_FLAG_THIN_LENS is told on the host, on the CPU: the refusals of the request
(rt_amd/csrc/frame_setup.cpp), the check against the context's lens and the frame's camera (rt_amd/csrc/lens.cpp), its launch plan
(rt_amd/csrc/launch_plan.cpp) and the flag's refusal by passes (progressive.cpp: progressive and adaptive frames).
tests/native/lens_plan_dump.cpp is built with g++ alone; every request below must come out as tests/golden/launch_plans_lens.txt says
(`python -m tests.test_lens_plan` writes that file)."""
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import pytest

from rt_amd import capi
from tests import pass_plan
from tests.conftest import GOLDEN, ROOT

SOURCES = [str(ROOT / "tests" / "native" / "lens_plan_dump.cpp"), str(ROOT / "rt_amd" / "csrc" / "launch_plan.cpp"), str(ROOT / "rt_amd" / "csrc" / "frame_setup.cpp"), str(ROOT / "rt_amd" / "csrc" / "lens.cpp")]
GOLDEN_PLANS = GOLDEN / "launch_plans_lens.txt"
LENS = capi.RT_HIP_FLAG_THIN_LENS
SM = capi.RT_HIP_FLAG_SM_MATERIALS
KERNEL = {name: code for code, name in capi.KERNEL_NAMES.items()}
INVALID_ARGUMENT, UNSUPPORTED = 1, 5
PINHOLE, PLAIN_EYE, GUARDED_EYE, NO_EYE = 0, 1, 2, 3

REFUSED_WITH = {
    "fast": capi.RT_HIP_FLAG_FAST,
    "force_tiled": capi.RT_HIP_FLAG_FORCE_TILED,
    "force_resident": capi.RT_HIP_FLAG_FORCE_RESIDENT,
    "force_streamed": capi.RT_HIP_FLAG_FORCE_STREAMED,
    "force_half_chunks": capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS,
    "trace_boxes": capi.RT_HIP_FLAG_TRACE_BOXES,
    "box_bvh": capi.RT_HIP_FLAG_TRACE_BOXES | capi.RT_HIP_FLAG_BOX_BVH,
    "emission": capi.RT_HIP_FLAG_EMISSION,
    "direct_light": capi.RT_HIP_FLAG_EMISSION | capi.RT_HIP_FLAG_DIRECT_LIGHT,
}
ACCEPTED_WITH = {
    "stats": capi.RT_HIP_FLAG_STATS,
    "persistent_frame": capi.RT_HIP_FLAG_PERSISTENT_FRAME,
    "whole_chunks": capi.RT_HIP_FLAG_FORCE_WHOLE_CHUNKS,
}


def request(spheres, planes, flags=LENS, frame=(96, 54), spp=20, camera=PINHOLE, host=0, have_lens=1, aperture=0.05):
    return (spheres, planes, frame[0], frame[1], spp, camera, flags, host, have_lens, aperture)


# name -> request (n_spheres n_planes width local_rows samples_per_pixel camera flags host_frame have_lens aperture_radius)
CASES = {
    "small_scene": request(4, 1),
    "small_scene_sm": request(4, 1, flags=LENS | SM),
    "small_scene_flagless": request(4, 1, flags=0),
    "small_scene_no_aperture": request(4, 1, aperture=0.0),
    "small_scene_no_aperture_sm": request(4, 1, flags=LENS | SM, aperture=0.0),
    "small_scene_flagless_sm": request(4, 1, flags=SM),
    "lens_without_flag": request(4, 1, flags=0, aperture=0.3),
    "tilted_camera": request(4, 1, camera=PLAIN_EYE),
    "tilted_camera_sm": request(4, 1, camera=PLAIN_EYE, flags=LENS | SM),
    "guarded_eye_camera": request(4, 1, camera=GUARDED_EYE),
    "scalar_load_scan_40_spheres": request(40, 1),
    "scalar_load_scan_40_spheres_sm": request(40, 1, flags=LENS | SM),
    "lds_scan_39_spheres": request(39, 1),
    "bvh_flag_200_spheres": request(200, 1, flags=LENS | capi.RT_HIP_FLAG_BVH),
    "bvh_flag_200_spheres_sm": request(200, 1, flags=LENS | capi.RT_HIP_FLAG_BVH | SM),
    "bvh_device_build": request(200, 1, flags=LENS | capi.RT_HIP_FLAG_BVH | capi.RT_HIP_FLAG_BVH_DEVICE_BUILD),
    "resident_1300_primitives": request(1300, 0, frame=(1920, 1080), spp=64),
    "hierarchy_1301_primitives": request(1300, 1, frame=(32, 18), spp=16),
    "hierarchy_1301_primitives_flagless": request(1300, 1, frame=(32, 18), spp=16, flags=0),
    "hierarchy_1301_primitives_no_aperture": request(1300, 1, frame=(32, 18), spp=16, aperture=0.0),
    "headline_frame_host": request(4, 1, frame=(1920, 1080), spp=64, host=1),
    "headline_frame_host_flagless": request(4, 1, frame=(1920, 1080), spp=64, host=1, flags=0),
    "headline_frame_host_no_aperture": request(4, 1, frame=(1920, 1080), spp=64, host=1, aperture=0.0),
    "preview_ignores_it": request(4, 1, flags=LENS | capi.RT_HIP_FLAG_PREVIEW, have_lens=0),
    "no_lens": request(4, 1, have_lens=0),
    "no_eye": request(4, 1, camera=NO_EYE),
    "no_eye_no_aperture": request(4, 1, camera=NO_EYE, aperture=0.0),
    "lds_too_small": request(200, 1, flags=LENS | capi.RT_HIP_FLAG_BVH, frame=(1920, 1080), spp=3424),
    **{f"with_{name}": request(4, 1, flags=LENS | bit) for name, bit in REFUSED_WITH.items()},
    **{f"with_{name}_no_aperture": request(4, 1, flags=LENS | bit, aperture=0.0) for name, bit in REFUSED_WITH.items()},
    **{f"with_{name}": request(4, 1, flags=LENS | bit) for name, bit in ACCEPTED_WITH.items()},
    **{f"bit_{bit}": request(4, 1, flags=LENS | (1 << bit)) for bit in (12, 15, 20, 31)},
}


def ask(directory):
    cxx = shutil.which("g++")
    if cxx is None:
        return None
    exe = Path(directory) / "lens_plan_dump"
    built = subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *SOURCES, "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    out = subprocess.run([str(exe)], input="".join(" ".join(str(v) for v in r) + "\n" for r in CASES.values()), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(CASES)
    return dict(zip(CASES, lines))


def table_of(answers):
    return "".join(f"{name}: {' '.join(str(v) for v in CASES[name])} -> {line}\n" for name, line in answers.items())


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    got = ask(tmp_path_factory.mktemp("lens_plan"))
    if got is None:
        pytest.skip("no g++")
    return got


def fields(line):
    assert not line.startswith("refused"), line
    return {k: int(v) for k, v in (f.split("=") for f in line.split())}


def test_every_plan_is_the_golden_one(answers):
    assert table_of(answers) == GOLDEN_PLANS.read_text(), "the plans of lens frames moved: if that is meant, write the new table to tests/golden/launch_plans_lens.txt"


def build_of(plan):
    return (plan["variant"], plan["scan"], plan["planes"], plan["general_camera"], plan["sm_table"], plan["lens"])


def test_the_eight_lens_builds_are_reached_by_the_requests_one_expects(answers):
    resident, bvh = KERNEL["resident"], KERNEL["bvh"]
    want = {
        "small_scene": (resident, 0, 0, 0, 0, 1),  # (not the scalar-register kernel the flag-less frame takes)
        "small_scene_sm": (resident, 0, 0, 0, 1, 1),
        "tilted_camera": (resident, 0, 0, 1, 0, 1),
        "tilted_camera_sm": (resident, 0, 0, 1, 1, 1),
        "scalar_load_scan_40_spheres": (resident, 0, 1, 0, 0, 1),
        "scalar_load_scan_40_spheres_sm": (resident, 0, 1, 0, 1, 1),
        "bvh_flag_200_spheres": (bvh, -4, 0, 0, 0, 1),
        "bvh_flag_200_spheres_sm": (bvh, -4, 0, 0, 1, 1),
    }
    for name, build in want.items():
        assert build_of(fields(answers[name])) == build, name
    assert len(set(want.values())) == 8
    assert build_of(fields(answers["guarded_eye_camera"])) == want["tilted_camera"]
    assert build_of(fields(answers["lds_scan_39_spheres"])) == want["small_scene"]
    assert build_of(fields(answers["bvh_device_build"])) == want["bvh_flag_200_spheres"]
    assert build_of(fields(answers["hierarchy_1301_primitives"])) == want["bvh_flag_200_spheres"]  # (the flag-less frame takes the streamed kernel)
    assert fields(answers["hierarchy_1301_primitives_flagless"])["variant"] == KERNEL["streamed"]
    assert build_of(fields(answers["resident_1300_primitives"])) == want["scalar_load_scan_40_spheres"]
    assert fields(answers["small_scene_flagless"])["variant"] == KERNEL["small"]
    assert fields(answers["small_scene"])["table_bytes"] == (4 + 1) * 16 and fields(answers["scalar_load_scan_40_spheres"])["table_bytes"] == 16 and fields(answers["bvh_flag_200_spheres"])["table_bytes"] == 24 * 1024
    for name, line in answers.items():
        if not line.startswith("refused") and fields(line)["lens"]:
            plan = fields(line)
            assert plan["halves"] == plan["sub_chunk_items"] == plan["big_scene"] == plan["pass"] == plan["boxes"] == plan["lights"] == 0 and plan["persistent_slot"] == -1, name
            assert plan["lds_bytes"] == plan["table_bytes"] + plan["slot_bytes"] <= 64 * 1024, name
            assert plan["band_offered"] == 0, name  # a lens frame never takes the sky band
    for name in ACCEPTED_WITH:
        assert build_of(fields(answers[f"with_{name}"])) == want["small_scene"], name


def test_without_an_aperture_the_flag_changes_nothing(answers):
    """byte for byte: the plan of the flag with a lens of radius 0 is the flag-less plan, the offer of a sky band included"""
    assert answers["small_scene_no_aperture"] == answers["small_scene_flagless"] == answers["lens_without_flag"]
    assert answers["small_scene_no_aperture_sm"] == answers["small_scene_flagless_sm"]
    assert answers["hierarchy_1301_primitives_no_aperture"] == answers["hierarchy_1301_primitives_flagless"]
    assert answers["headline_frame_host_no_aperture"] == answers["headline_frame_host_flagless"]
    assert "band_offered=1" in answers["small_scene_no_aperture"] and "lens=0" in answers["small_scene_no_aperture"]
    assert "lens=0" in answers["preview_ignores_it"]  # (and no lens is asked for)


def test_refusals_name_the_flag(answers):
    for name in REFUSED_WITH:
        for case in (f"with_{name}", f"with_{name}_no_aperture"):
            assert answers[case].startswith(f"refused {UNSUPPORTED} rt_hip_render_device: RT_HIP_FLAG_THIN_LENS "), answers[case]
    assert "RT_HIP_FLAG_FAST" in answers["with_fast"] and "RT_HIP_FLAG_FORCE_HALF_CHUNKS" in answers["with_force_half_chunks"]
    for name in ("force_tiled", "force_resident", "force_streamed"):
        assert "RT_HIP_FLAG_FORCE_TILED / _RESIDENT / _STREAMED" in answers[f"with_{name}"]
    for name in ("trace_boxes", "box_bvh"):
        assert "RT_HIP_FLAG_TRACE_BOXES / RT_HIP_FLAG_BOX_BVH" in answers[f"with_{name}"]
    for name in ("emission", "direct_light"):
        assert "RT_HIP_FLAG_EMISSION / RT_HIP_FLAG_DIRECT_LIGHT" in answers[f"with_{name}"]
    assert answers["no_lens"] == f"refused {INVALID_ARGUMENT} rt_hip_render_device: RT_HIP_FLAG_THIN_LENS without a lens (rt_hip_set_lens)"
    for case in ("no_eye", "no_eye_no_aperture"):  # a lens needs a perspective matrix, whatever its radius
        assert answers[case].startswith(f"refused {UNSUPPORTED} rt_hip_render_device: RT_HIP_FLAG_THIN_LENS ") and "perspective matrix" in answers[case]
    for bit in (12, 15, 20, 31):
        assert answers[f"bit_{bit}"].startswith(f"refused {UNSUPPORTED} rt_hip_render_device: unknown flag bits"), bit


def test_the_plans_lds_is_checked_against_the_device_limit(answers):
    """the hierarchy kernel's lens build: 24 KiB of stacks in front of the chunk sums, as every build of it (tests/test_plan_lds_limit.py's rule)"""
    line = answers["lds_too_small"]
    assert line.startswith(f"refused {UNSUPPORTED} rt_hip_render_device: ") and "LDS" in line and "at most 3408 samples fit" in line


def test_passes_refuse_the_flag_by_name():
    """progressive and adaptive frames: both go through refused_pass_flag (adaptive.hpp: refused_adaptive_flag is it)"""
    if pass_plan.executable() is None:
        pytest.skip("no g++")
    assert pass_plan.refused_flag(LENS) == "RT_HIP_FLAG_THIN_LENS"
    assert pass_plan.refused_flag(LENS | SM | capi.RT_HIP_FLAG_BVH) == "RT_HIP_FLAG_THIN_LENS"
    for bit in (12, 15, 20, 31):
        assert pass_plan.refused_flag(1 << bit) == "unknown flag bits"


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as scratch:
        made = ask(scratch)
    if made is None:
        sys.exit("no g++")
    GOLDEN_PLANS.write_text(table_of(made))
    print(f"wrote {GOLDEN_PLANS}")
