"""tests/native/light_sweep_plan_dump.cpp, built once per test process: plan_launch asked on the CPU for frames with RT_HIP_FLAG_EMISSION /
RT_HIP_FLAG_DIRECT_LIGHT — which of the sixteen light builds a frame takes, its chunk count, tile and fold path.  TEST INFRASTRUCTURE,
shared by tests/test_light_rare_branches.py, tests/test_gpu_light_rare_branches.py and tests/test_gpu_light_chunk_sweep.py: a test asks
it BEFORE it renders and asserts the answer, so that a later change of policy cannot silently empty a case."""
import functools
import shutil
import subprocess
import tempfile

from oracle import binding as oracle
from rt_amd import capi
from tests import direct_reference as direct_ref
from tests.conftest import ROOT

SOURCES = [str(ROOT / "tests" / "native" / "light_sweep_plan_dump.cpp"), str(ROOT / "rt_amd" / "csrc" / "launch_plan.cpp")]
INTEGERS = ("variant big_scene chunks pixels_log2 tile_w_log2 tiles_x tiles_y halves scan planes general_camera sub_chunk_items sm_table pass boxes lights direct grid_x grid_y table_bytes slot_bytes "
            "lds_bytes total_items").split()
EMISSION = capi.RT_HIP_FLAG_EMISSION
DIRECT = capi.RT_HIP_FLAG_EMISSION | capi.RT_HIP_FLAG_DIRECT_LIGHT
SM = capi.RT_HIP_FLAG_SM_MATERIALS
BVH = capi.RT_HIP_FLAG_BVH
DEVICE_BUILD = capi.RT_HIP_FLAG_BVH_DEVICE_BUILD
# What the MI355X gives a workgroup (tests/test_gpu_chunk_sweep.py holds the figure to the device): the context plans under it.
DEVICE_LDS = 160 * 1024
SCANS = ("LDS scan, pinhole", "LDS scan, general camera", "scalar-load scan", "hierarchy")
# the sixteen builds, as build_name spells them
BUILDS = {flag: [f"{flag} ({scan}, {table})" for scan in SCANS for table in ("mg", "sm")] for flag in ("lights", "direct")}


@functools.lru_cache(maxsize=None)
def executable():
    """The dump program, built with g++ alone (nothing of ROCm on the command line)."""
    cxx = shutil.which("g++")
    assert cxx is not None, "the plan dump program needs g++: without it nothing says which build a frame takes"
    exe = tempfile.mkdtemp(prefix="light_plan_") + "/light_sweep_plan_dump"
    built = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *SOURCES, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


@functools.lru_cache(maxsize=None)
def ask(request):
    out = subprocess.run([executable()], input=" ".join(str(v) for v in request) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    fields, _, refusal = out.stdout.rstrip("\n").partition(" refusal=")
    plan = {k: int(v) for k, v in (field.split("=") for field in fields.split())}
    assert list(plan) == INTEGERS
    plan["refusal"] = refusal
    return plan


def camera_of(pod, width, height):
    return 0 if oracle.primary_ray(pod, width, height, 0, 0, want_form=True)[2] == "pinhole" else 2


def light_counts(pod, table):
    """(materials that are lights, sampled lights of the scene) under `table`, as the context counts them"""
    return int((table > 0).any(axis=1).sum()), direct_ref.count(pod, table)


def planned(pod, table, width, height, flags, host):
    """plan_launch as render.hip asks it for `pod` under the emission table: `flags` are the call's, `host` the entry point's host_frame
    (1: rt_hip_render's page-locked frame, 0: rt_hip_render_device's tensor).  A dict of the plan's fields; "refusal" is its text."""
    n_lights, n_sampled = light_counts(pod, table)
    return dict(ask((pod.n_spheres, pod.n_planes, width, height, pod.samples_per_pixel, camera_of(pod, width, height), flags & ~DEVICE_BUILD, host, n_lights, n_sampled, DEVICE_LDS)))


def build_name(p):
    """One of BUILDS' names for a plan of a light or direct build"""
    assert p["lights"] and p["scan"] in (0, -4) and not (p["halves"] or p["sub_chunk_items"] or p["pass"] or p["boxes"] or p["big_scene"]), p
    scan = "hierarchy" if p["scan"] == -4 else "scalar-load scan" if p["planes"] else "LDS scan, general camera" if p["general_camera"] else "LDS scan, pinhole"
    return f"{'direct' if p['direct'] else 'lights'} ({scan}, {'sm' if p['sm_table'] else 'mg'})"


def fold_path(p):
    """How fold_tile folds a tile of 2^pixels_log2 pixels: one channel per lane where three lanes per pixel fit a wave, else one pixel per lane."""
    return "channel-per-lane" if (3 << p["pixels_log2"]) <= 64 else "per-pixel"


def kernel_of(p):
    return capi.KERNEL_NAMES[p["variant"]]
