"""tests/native/lds_plan_dump.cpp, built once per test process: plan_launch asked on the CPU with every field of a launch_request, the
device's per-workgroup LDS limit among them.  Shared by tests/test_plan_lds_limit.py, which pins that no plan stands that the limit
does not hold, and tests/test_gpu_chunk_sweep.py, which asks it which build, tile shape and fold path every one of its frames takes."""
import functools
import shutil
import subprocess
import tempfile

from tests.conftest import ROOT

SOURCES = [str(ROOT / "tests" / "native" / "lds_plan_dump.cpp"), str(ROOT / "rt_amd" / "csrc" / "launch_plan.cpp")]
INTEGERS = ("variant big_scene chunks pixels_log2 tile_w_log2 tiles_x tiles_y halves scan planes general_camera sub_chunk_items sm_table pass boxes box_tree adaptive grid_x grid_y table_bytes slot_bytes "
            "lds_bytes total_items first_chunk max_slot_bytes default_lds_limit").split()


@functools.lru_cache(maxsize=None)
def executable():
    """The dump program, built with g++ alone (nothing of ROCm on the command line); None without a compiler."""
    cxx = shutil.which("g++")
    if cxx is None:
        return None
    exe = tempfile.mkdtemp(prefix="lds_plan_") + "/lds_plan_dump"
    built = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *SOURCES, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def request(n_spheres, n_planes, width, height, spp, *, n_boxes=0, camera=0, flags=0, host_frame=0, pass_first=0, pass_samples=0, adaptive=0, lds_limit=0):
    return (n_spheres, n_planes, n_boxes, width, height, spp, camera, flags, host_frame, pass_first, pass_samples, adaptive, lds_limit)


def plans(requests):
    """requests: tuples as request() makes them -> one dict of the launch_plan's fields each; "refusal" is the plan's text ("" where it stands)."""
    assert executable() is not None, "the plan dump program needs g++: without it nothing says which build and which fold path a frame takes"
    out = subprocess.run([executable()], input="".join(" ".join(str(v) for v in r) + "\n" for r in requests), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(requests)
    result = []
    for line in lines:
        fields, _, refusal = line.partition(" refusal=")
        plan = {k: int(v) for k, v in (field.split("=") for field in fields.split())}
        assert list(plan) == INTEGERS
        plan["refusal"] = refusal
        result.append(plan)
    return result


def plan(*args, **kwargs):
    return plans([request(*args, **kwargs)])[0]


def fold_path(plan):
    """How fold_tile folds a tile of 2^pixels_log2 pixels: one channel per lane where three lanes per pixel fit a wave, else one pixel per lane."""
    return "channel-per-lane" if (3 << plan["pixels_log2"]) <= 64 else "per-pixel"
