"""The host-only policy of progressive frames on the CPU: the launch plan of a pass (rt_amd/csrc/launch_plan.cpp), the sequencing of
passes and the flags a pass takes (rt_amd/csrc/progressive.cpp).  tests/native/pass_plan_dump.cpp is built with g++ alone — nothing
of ROCm on the command line.  A wrong plan costs a frame its bits (a pass through a kernel that has no pass build, a first chunk
that is not the accumulation's), a wrong sequence costs samples: both are pinned here, where no GPU is needed to see them."""
import itertools

import pytest

from rt_amd import capi
from tests import pass_plan

KERNEL = {name: code for code, name in capi.KERNEL_NAMES.items()}
SPHERES = [1, 8, 9, 39, 40, 1024, 1301, 100000]
PLANES = [0, 1, 4]
FRAMES = [(37, 23), (1920, 1080)]
PASSES = [(0, 16), (16, 16), (32, 48), (96, 4), (0, 100), (64, 512), (4096, 4096)]  # (first_sample, n_samples)


@pytest.fixture(scope="module", autouse=True)
def _compiler():
    if pass_plan.executable() is None:
        pytest.skip("no g++")


def request(spheres, planes, frame=(1920, 1080), spp=8192, camera=0, flags=0, host=0, first=0, n=0, tame=1):
    return (spheres, planes, tame, frame[0], frame[1], spp, camera, flags, host, 0, first, n)


def test_pass_plans_take_the_tile_per_wave_whole_chunk_kernels():
    """Never SMALL, STREAMED or TILED; whole chunks; the queue is the PASS's; the first chunk is the accumulation's."""
    cases = [(s, p, frame, camera, flags, host, first, n) for s in SPHERES for p in PLANES for frame in FRAMES for camera in (0, 1, 2) for flags in (0, capi.RT_HIP_FLAG_SM_MATERIALS, capi.RT_HIP_FLAG_BVH) for host in (0, 1)
             for first, n in PASSES]
    plans = pass_plan.plans([request(s, p, frame, camera=camera, flags=flags, host=host, first=first, n=n) for s, p, frame, camera, flags, host, first, n in cases])
    families = set()
    for (s, p, frame, camera, flags, host, first, n), plan in zip(cases, plans):
        where = str(((s, p, frame, camera, flags, host, first, n), plan))
        assert plan["variant"] in (KERNEL["resident"], KERNEL["bvh"]), where
        assert plan["pass"] == 1 and plan["big_scene"] == 0 and plan["persistent_slot"] == -1, where
        assert plan["halves"] == 0 and plan["sub_chunk_items"] == 0, where
        assert plan["chunks"] == -(-n // 16), where
        assert plan["first_chunk"] == first // 16, where
        assert plan["scan"] == (-4 if plan["variant"] == KERNEL["bvh"] else 0), where
        assert plan["sm_table"] == (1 if flags & capi.RT_HIP_FLAG_SM_MATERIALS else 0), where
        # the tiles cover the rows, four per workgroup; the slots are the four tiles' chunk sums
        assert (plan["tiles_x"] << plan["tile_w_log2"]) >= frame[0] and (plan["tiles_y"] << (plan["pixels_log2"] - plan["tile_w_log2"])) >= frame[1], where
        assert (plan["grid_x"], plan["grid_y"]) == ((plan["tiles_x"] + 3) // 4, plan["tiles_y"]), where
        assert plan["slot_bytes"] == 4 * (plan["chunks"] << plan["pixels_log2"]) * 12 and plan["lds_bytes"] == plan["table_bytes"] + plan["slot_bytes"], where
        assert plan["item_sums_bytes"] == plan["pixel_done_bytes"] == 0, where  # (the accumulator travels in pixel_done's place: nothing of the rolling kernels' is prepared)
        assert plan["block_items"] == plan["lane_cap"] == plan["sparse_rays"] == plan["item_samples"] == 0, where  # (block_items carries first_chunk at launch: the plan leaves it alone)
        if n <= 4096:  # what the API accepts: one pass fits the LDS slots
            assert plan["slot_bytes"] <= 48 * 1024, where
        families.add((plan["scan"], plan["planes"], plan["general_camera"], plan["sm_table"]))
    # every pass build there is: the resident kernel's three and the hierarchy's, with and without the sm table
    assert families == {(scan, planes, gc, sm) for scan, planes, gc in [(0, 0, 0), (0, 0, 1), (0, 1, 0), (-4, 0, 0)] for sm in (0, 1)}


def test_the_family_is_the_hierarchy_for_the_flag_and_for_scenes_of_the_streamed_kernels_size():
    for frame, spp in [((37, 23), 40), ((1920, 1080), 64)]:
        scenes = list(itertools.product(SPHERES, PLANES))
        one_shot = pass_plan.plans([request(s, p, frame, spp=spp) for s, p in scenes])
        for flags in (0, capi.RT_HIP_FLAG_BVH):
            passes = pass_plan.plans([request(s, p, frame, spp=spp, flags=flags, first=16, n=16) for s, p in scenes])
            for (s, p), whole, plan in zip(scenes, one_shot, passes):
                streamed_size = whole["variant"] == KERNEL["streamed"]
                assert plan["variant"] == (KERNEL["bvh"] if flags or streamed_size else KERNEL["resident"]), (s, p, frame, flags)
                # the rule in numbers, where it does not depend on the frame: up to 1024 primitives resident, above 1300 the hierarchy
                if s + p <= 1024 and not flags:
                    assert plan["variant"] == KERNEL["resident"], (s, p)
                if s + p > 1300:
                    assert plan["variant"] == KERNEL["bvh"], (s, p)
                if plan["variant"] == KERNEL["resident"]:  # ... and which scan of the resident kernel: the scalar-load one from 40 spheres
                    assert plan["planes"] == (1 if s >= 40 else 0) and plan["table_bytes"] == 16 * ((s if s < 40 else 0) + p), (s, p)
    # a scene the one-shot path gives to the scalar-register kernel takes the resident one, as under RT_HIP_FLAG_FORCE_RESIDENT
    (small,) = pass_plan.plans([request(4, 1)])
    (forced,) = pass_plan.plans([request(4, 1, flags=capi.RT_HIP_FLAG_FORCE_RESIDENT)])
    (as_pass,) = pass_plan.plans([request(4, 1, n=16)])
    assert small["variant"] == KERNEL["small"] and forced["variant"] == as_pass["variant"] == KERNEL["resident"]
    assert (as_pass["scan"], as_pass["planes"], as_pass["general_camera"], as_pass["table_bytes"]) == (forced["scan"], forced["planes"], forced["general_camera"], forced["table_bytes"])


def test_the_tile_shapes_the_gpu_test_counts_on():
    """A 37 x 23 frame: passes of 16, 32 and 48 samples take tiles of 64, 32 and 16 pixels — the per-pixel fold twice, then one channel per lane."""
    plans = pass_plan.plans([request(4, 1, (37, 23), spp=100, host=1, first=0, n=n) for n in (16, 32, 48)])
    assert [p["pixels_log2"] for p in plans] == [6, 5, 4]
    assert [3 << p["pixels_log2"] <= 64 for p in plans] == [False, False, True]  # (fold_tile's test for the channel-per-lane path)


def test_a_request_without_a_pass_is_planned_as_ever(tmp_path):
    """Both pass fields 0: every field of the plan equals that of the same request built WITHOUT them — by tests/native/launch_plan_dump.cpp,
    which has never heard of passes and leaves the two fields to their defaults."""
    import shutil
    import subprocess

    from tests.conftest import ROOT

    exe = tmp_path / "launch_plan_dump"
    built = subprocess.run([shutil.which("g++"), "-std=c++17", "-O2", str(ROOT / "tests" / "native" / "launch_plan_dump.cpp"), str(ROOT / "rt_amd" / "csrc" / "launch_plan.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    requests = [request(s, p, frame, spp=spp, camera=camera, flags=flags) for s, p in [(4, 0), (4, 1), (12, 1), (700, 2), (2000, 0), (100000, 0)] for frame in FRAMES for spp in (1, 64, 100, 4096) for camera in (0, 2)
                for flags in (0, capi.RT_HIP_FLAG_BVH, capi.RT_HIP_FLAG_FORCE_TILED, capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS)]
    out = subprocess.run([str(exe)], input="".join(" ".join(str(v) for v in r[:10]) + "\n" for r in requests), capture_output=True, text=True, check=True).stdout.splitlines()
    names = [n for n in out[0][2:].split() if n != "|"]
    without = [dict(zip(names, (int(v) for v in line.split() if v != "|"))) for line in out[1:]]
    plans = pass_plan.plans(requests)
    assert len(without) == len(plans) == len(requests)
    for old, new in zip(without, plans):
        assert new["pass"] == 0 and new["first_chunk"] == 0
        shared = [name for name in new if name not in ("pass", "first_chunk")]
        assert len(shared) == 27 and all(name in old for name in shared)  # every field launch_plan had before there were passes
        assert {name: old[name] for name in shared} == {name: new[name] for name in shared}, (old, new)
    assert {p["variant"] for p in plans} == {KERNEL["small"], KERNEL["resident"], KERNEL["streamed"], KERNEL["tiled"], KERNEL["bvh"]}
    assert any(p["halves"] for p in plans)
    # pass_first_sample alone (pass_samples = 0) is no pass either: the same plan
    assert pass_plan.plans([r[:10] + (16, 0) for r in requests]) == plans


def test_next_pass_rounds_up_clamps_and_completes():
    key = pass_plan.key(spp=100)
    assert pass_plan.next_pass(False, 0, key, key, 16) == (True, 0, 16, False)  # nothing in flight: a new accumulation
    assert pass_plan.next_pass(True, 16, key, key, 16) == (False, 16, 16, False)
    assert pass_plan.next_pass(True, 16, key, key, 1) == (False, 16, 16, False)  # rounded up to a whole chunk
    assert pass_plan.next_pass(True, 16, key, key, 17) == (False, 16, 32, False)
    assert pass_plan.next_pass(True, 64, key, key, 48) == (False, 64, 36, True)  # clamped at the end: 100 is no multiple of 16
    assert pass_plan.next_pass(True, 96, key, key, 16) == (False, 96, 4, True)
    assert pass_plan.next_pass(True, 32, key, key, 0) == (False, 32, 68, True)  # 0: all that is left
    assert pass_plan.next_pass(False, 0, key, key, 0) == (True, 0, 100, True)
    assert pass_plan.next_pass(True, 100, key, key, 16) == (False, 100, 0, True)  # finished: nothing to launch
    assert pass_plan.next_pass(True, 100, key, key, 0) == (False, 100, 0, True)
    assert pass_plan.next_pass(True, 0, key, key, 0xFFFFFFFF) == (False, 0, 100, True)  # (no overflow in the rounding)
    small = pass_plan.key(spp=5)
    assert pass_plan.next_pass(False, 0, small, small, 16) == (True, 0, 5, True)
    whole = pass_plan.key(spp=64)
    assert [pass_plan.next_pass(True, done, whole, whole, 32) for done in (0, 32, 64)] == [(False, 0, 32, False), (False, 32, 32, True), (False, 64, 0, True)]


@pytest.mark.parametrize("field", ["fingerprint", "spp", "bounces", "width", "height", "seed", "flags"] + [f"matrix{i}" for i in range(16)])
def test_any_single_field_of_the_key_restarts(field):
    state = pass_plan.key(spp=100)
    if field.startswith("matrix"):
        matrix = list(range(1, 17))
        matrix[int(field[6:])] ^= 0x80000000  # one bit of one word: the sign
        changed = pass_plan.key(spp=100, matrix=tuple(matrix))
    else:
        changed = pass_plan.key(**{"spp": 100, field: {"fingerprint": 12, "spp": 116, "bounces": 6, "width": 38, "height": 24, "seed": 8, "flags": capi.RT_HIP_FLAG_SM_MATERIALS}[field]})
    restart, first, n, complete = pass_plan.next_pass(True, 48, state, changed, 16)
    assert (restart, first, n, complete) == (True, 0, 16, False)
    assert pass_plan.next_pass(True, 48, state, state, 16) == (False, 48, 16, False)  # (and the same key goes on)
    # a finished accumulation whose key changes starts again too
    assert pass_plan.next_pass(True, 100, state, changed, 16)[:3] == (True, 0, 16)


def test_the_flags_a_pass_takes():
    accepted = [0, capi.RT_HIP_FLAG_SM_MATERIALS, capi.RT_HIP_FLAG_BVH, capi.RT_HIP_FLAG_BVH | capi.RT_HIP_FLAG_BVH_DEVICE_BUILD, capi.RT_HIP_FLAG_BVH | capi.RT_HIP_FLAG_SM_MATERIALS]
    for flags in accepted:
        assert pass_plan.refused_flag(flags) is None
        assert pass_plan.refused_flag(flags | capi.RT_HIP_FLAG_STATS) is None  # (both entry points take it)
    for name in ["FAST", "PREVIEW", "FORCE_TILED", "FORCE_RESIDENT", "FORCE_STREAMED", "FORCE_HALF_CHUNKS", "FORCE_WHOLE_CHUNKS", "PERSISTENT_FRAME"]:
        assert pass_plan.refused_flag(getattr(capi, "RT_HIP_FLAG_" + name) | capi.RT_HIP_FLAG_BVH) == "RT_HIP_FLAG_" + name
        assert pass_plan.refused_flag(getattr(capi, "RT_HIP_FLAG_" + name) | capi.RT_HIP_FLAG_STATS) == "RT_HIP_FLAG_" + name
    assert pass_plan.refused_flag(1 << 12) == "unknown flag bits" and pass_plan.refused_flag(1 << 31) == "unknown flag bits"
