"""Adaptive sampling's host-only unit on the CPU (rt_amd/csrc/adaptive.cpp): the defaults, every refusal of the
parameter check, every restart condition of the sequencing, completion by the cap and by "no pixel active", the short last pass, the
flags an adaptive pass takes, and the launch plan of an adaptive pass (rt_amd/csrc/launch_plan.cpp).  tests/native/adaptive_plan_dump.cpp
is built with g++ alone — nothing of ROCm on the command line.  Of the plans every other launch gets this file re-runs ONE table: the
grid of tests/test_launch_plan.py through the existing dump program against tests/golden/launch_plans.txt, and a pass's plan against an
adaptive pass's.  tests/golden/launch_plans_boxes.txt and the pass-plan dump are held by the files that always held them
(tests/test_box_plan.py, tests/test_box_bvh_plan.py, tests/test_pass_plan.py), which this change leaves as they are."""
import shutil
import subprocess

import pytest

from rt_amd import capi
from tests import adaptive_plan
from tests import test_launch_plan as launch_plans

KERNEL = {name: code for code, name in capi.KERNEL_NAMES.items()}
NAN_WORD, INF_WORD, NEG_ZERO_WORD = 0x7FC00000, 0x7F800000, 0x80000000


@pytest.fixture(scope="module", autouse=True)
def _compiler():
    if adaptive_plan.executable() is None:
        pytest.skip("no g++")


def test_the_defaults():
    threshold, floor, min_samples = adaptive_plan.defaults()
    assert (threshold, floor, min_samples) == (pytest.approx(0.03, rel=1e-7), pytest.approx(0.01, rel=1e-7), 32)
    assert adaptive_plan.check(threshold, floor, min_samples, 16) == (0, None)


def test_the_pass_size_is_rounded_up_to_whole_chunks():
    assert [adaptive_plan.pass_size(n) for n in (0, 1, 16, 17, 48, 4095, 0xFFFFFFFF)] == [16, 16, 16, 32, 48, 4096, 1 << 32]


@pytest.mark.parametrize("field,values", [("threshold", [-1.0, -1e-30, NAN_WORD, INF_WORD, 0xFF800000]), ("floor", [-0.5, NAN_WORD, INF_WORD])])
def test_a_threshold_or_floor_that_is_not_finite_and_non_negative_is_refused_by_name(field, values):
    for value in values:
        args = {"threshold": 0.03, "floor": 0.01}
        args[field] = value
        status, message = adaptive_plan.check(args["threshold"], args["floor"], 32, 16)
        assert status == 1 and f"rt_hip_adaptive_params: {field} " in message, (value, message)


def test_zero_and_large_values_are_accepted():
    for threshold, floor in [(0.0, 0.0), (NEG_ZERO_WORD, 0.0), (1e30, 1e30), (3.0e38, 0.0)]:
        assert adaptive_plan.check(threshold, floor, 32, 16) == (0, None)


def test_min_samples_is_at_least_two_passes_and_may_lie_above_any_cap():
    for size, least in [(16, 32), (32, 64), (48, 96), (4096, 8192)]:
        assert adaptive_plan.check(0.03, 0.01, least, size) == (0, None)
        status, message = adaptive_plan.check(0.03, 0.01, least - 1, size)
        assert status == 1 and "min_samples" in message and str(size) in message
    assert adaptive_plan.check(0.03, 0.01, 0xFFFFFFFF, 16) == (0, None)
    assert adaptive_plan.check(0.03, 0.01, 0xFFFFFFFF, 1 << 32)[0] == 1  # (a pass size beyond 32 bits: nothing is at least two of those)


def test_nothing_in_flight_starts_at_sample_0():
    key = adaptive_plan.key()
    assert adaptive_plan.next_pass(False, 0, 0, key, key) == (True, 0, 16, True)
    assert adaptive_plan.next_pass(False, 64, 0, key, key) == (True, 0, 16, True)  # (whatever a failed pass left in the state)


def test_the_accumulation_goes_on_pass_by_pass():
    key = adaptive_plan.key(spp=128)
    for done in range(16, 128, 16):
        assert adaptive_plan.next_pass(True, done, 100, key, key) == (False, done, 16, True)
    key48 = adaptive_plan.key(spp=144, pass_samples=48, min_samples=96)
    assert adaptive_plan.next_pass(True, 96, 1, key48, key48) == (False, 96, 48, True)


CHANGES = {"fingerprint": 12, "spp": 256, "bounces": 6, "matrix": tuple(range(2, 18)), "width": 38, "height": 24, "seed": 8, "flags": capi.RT_HIP_FLAG_SM_MATERIALS, "threshold": 0.031, "floor": 0.0, "min_samples": 48,
           "pass_samples": 32}


@pytest.mark.parametrize("field", sorted(CHANGES))
def test_every_field_of_the_key_restarts(field):
    state = adaptive_plan.key(min_samples=64)
    wanted = adaptive_plan.key(**{"min_samples": 64, field: CHANGES[field]})
    restart, first, n, whole = adaptive_plan.next_pass(True, 64, 100, state, wanted)
    assert (restart, first) == (True, 0), field
    assert n == (32 if field == "pass_samples" else 16) and whole


def test_the_matrix_and_the_parameters_are_compared_as_bit_patterns():
    zero, negative_zero = adaptive_plan.key(floor=0.0), adaptive_plan.key(floor=-0.0)
    assert adaptive_plan.next_pass(True, 32, 5, zero, negative_zero)[0] is True
    assert adaptive_plan.next_pass(True, 32, 5, zero, zero)[0] is False


def test_completion_by_the_cap():
    key = adaptive_plan.key(spp=128)
    assert adaptive_plan.next_pass(True, 112, 9, key, key) == (False, 112, 16, True)
    assert adaptive_plan.next_pass(True, 128, 9, key, key) == (False, 128, 0, False)
    assert adaptive_plan.complete(128, 128, 9) and not adaptive_plan.complete(128, 112, 9)


def test_completion_by_no_pixel_active():
    key = adaptive_plan.key(spp=128)
    assert adaptive_plan.next_pass(True, 32, 0, key, key) == (False, 32, 0, False)
    assert adaptive_plan.complete(128, 32, 0) and not adaptive_plan.complete(128, 32, 1)
    # ... and a changed key starts again all the same
    assert adaptive_plan.next_pass(True, 32, 0, key, adaptive_plan.key(spp=128, seed=9)) == (True, 0, 16, True)


def test_the_short_last_pass():
    key = adaptive_plan.key(spp=40)
    assert adaptive_plan.next_pass(True, 32, 3, key, key) == (False, 32, 8, False)
    key = adaptive_plan.key(spp=100, pass_samples=48, min_samples=96)
    assert adaptive_plan.next_pass(True, 96, 3, key, key) == (False, 96, 4, False)
    key = adaptive_plan.key(spp=8)  # a cap below one pass: the first pass is the short last one
    assert adaptive_plan.next_pass(False, 0, 0, key, key) == (True, 0, 8, False)


def test_the_accepted_flags_are_exactly_the_passes():
    accepted = capi.RT_HIP_FLAG_SM_MATERIALS | capi.RT_HIP_FLAG_BVH | capi.RT_HIP_FLAG_BVH_DEVICE_BUILD | capi.RT_HIP_FLAG_STATS
    assert adaptive_plan.refused_flag(0) is None and adaptive_plan.refused_flag(accepted) is None
    for name in ("FAST", "PREVIEW", "FORCE_TILED", "FORCE_RESIDENT", "FORCE_STREAMED", "FORCE_HALF_CHUNKS", "FORCE_WHOLE_CHUNKS", "PERSISTENT_FRAME", "TRACE_BOXES", "BOX_BVH"):
        assert adaptive_plan.refused_flag(getattr(capi, "RT_HIP_FLAG_" + name) | accepted) == "RT_HIP_FLAG_" + name
    assert adaptive_plan.refused_flag(capi.RT_HIP_FLAG_TRACE_BOXES | capi.RT_HIP_FLAG_BOX_BVH) == "RT_HIP_FLAG_BOX_BVH"
    assert adaptive_plan.refused_flag(1 << 12) == "unknown flag bits"


SPHERES = [1, 8, 9, 39, 40, 1024, 1301, 100000]
FRAMES = [(37, 23), (1920, 1080), (3840, 2160), (8192, 4096)]


def test_adaptive_plans_take_the_adaptive_builds_and_tiles_of_at_most_64_pixels():
    cases = [(s, p, frame, camera, flags, first, n) for s in SPHERES for p in (0, 1, 4) for frame in FRAMES for camera in (0, 1, 2) for flags in (0, capi.RT_HIP_FLAG_SM_MATERIALS, capi.RT_HIP_FLAG_BVH)
             for first, n in [(0, 16), (16, 16), (32, 32), (96, 48), (128, 8), (0, 4096)]]
    plans = adaptive_plan.plans([(s, p, 1, frame[0], frame[1], 8192, camera, flags, first, n) for s, p, frame, camera, flags, first, n in cases])
    families = set()
    for (s, p, frame, camera, flags, first, n), plan in zip(cases, plans):
        where = str(((s, p, frame, camera, flags, first, n), plan))
        assert plan["variant"] in (KERNEL["resident"], KERNEL["bvh"]), where
        assert plan["pass"] == 1 and plan["adaptive"] == 1, where
        assert plan["scan_code"] == (-11 if plan["variant"] == KERNEL["bvh"] else -10), where
        assert plan["is_pass"] == 1 and plan["is_adaptive"] == 1 and plan["scan_of"] == plan["scan"] == (-4 if plan["variant"] == KERNEL["bvh"] else 0), where
        assert plan["chunks"] == -(-n // 16) and plan["first_chunk"] == first // 16, where
        assert plan["pixels_log2"] <= 6 and plan["tile_w_log2"] <= plan["pixels_log2"], where  # ONE 64-bit stop mask per wave
        assert (plan["tiles_x"] << plan["tile_w_log2"]) >= frame[0] and (plan["tiles_y"] << (plan["pixels_log2"] - plan["tile_w_log2"])) >= frame[1], where
        assert (plan["grid_x"], plan["grid_y"]) == ((plan["tiles_x"] + 3) // 4, plan["tiles_y"]), where
        assert plan["slot_bytes"] == 4 * (plan["chunks"] << plan["pixels_log2"]) * 12, where
        families.add((plan["scan_code"], plan["planes"], plan["general_camera"], plan["sm_table"]))
    # the eight adaptive builds: the resident kernel's three and the hierarchy's, with and without the sm table
    assert families == {(code, planes, gc, sm) for code, planes, gc in [(-10, 0, 0), (-10, 0, 1), (-10, 1, 0), (-11, 0, 0)] for sm in (0, 1)}


@pytest.mark.parametrize("n,pixels_log2", [(16, 6), (32, 5), (48, 4)])
def test_the_tile_of_a_small_frames_passes(n, pixels_log2):
    """37 x 23 through basic.toml's 4 spheres: what tests/test_gpu_adaptive.py relies on for its two fold paths."""
    (plan,) = adaptive_plan.plans([(4, 0, 1, 37, 23, 144, 0, 0, 0, n)])
    assert plan["pixels_log2"] == pixels_log2 and (3 << pixels_log2 <= 64) == (n == 48)


def test_an_adaptive_pass_is_planned_as_the_pass_it_is_except_for_tiles_beyond_64_pixels():
    """Field by field the plan of a pass, where that pass's tile has at most 64 pixels."""
    from tests import pass_plan

    for frame in FRAMES:
        for n in (16, 32, 48):
            (a,) = adaptive_plan.plans([(700, 2, 1, frame[0], frame[1], 256, 0, 0, 32, n)])
            (b,) = pass_plan.plans([(700, 2, 1, frame[0], frame[1], 256, 0, 0, 0, 0, 32, n)])
            if b["pixels_log2"] <= 6:
                assert all(a[k] == b[k] for k in a if k in b and k != "scan"), (frame, n)
            else:
                assert n == 16 and frame[0] * frame[1] >= 49152 * 128 and a["pixels_log2"] == 6  # (one-chunk passes of frames beyond 6M pixels)


def test_every_other_launch_is_planned_as_it_was(tmp_path):
    """tests/golden/launch_plans.txt, byte for byte, through the existing dump program."""
    exe = tmp_path / "launch_plan_dump"
    built = subprocess.run([shutil.which("g++"), "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *launch_plans.SOURCES, "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    requests = launch_plans.grid()
    out = subprocess.run([str(exe)], input="".join(" ".join(str(v) for v in r) + "\n" for r in requests), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout == launch_plans.GOLDEN.read_text()
