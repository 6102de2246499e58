"""Frames at the extremes of shape: the plan dump programs asked for them, and the case table of tests/test_gpu_extreme_shapes.py.
TEST INFRASTRUCTURE, shared by tests/test_plan_frame_extremes.py, which holds every accepted frame's grid in range on the CPU and the table
below to the plan, and tests/test_gpu_extreme_shapes.py, which renders the table.

The dump programs.  None is added: they are the ones tests/test_launch_plan.py, test_box_plan.py, test_light_plan.py, test_direct_plan.py
and test_sky_band_rule.py build, built the same way; passes and adaptive passes are asked through tests/pass_plan.py and
tests/adaptive_plan.py, the frames of the table through tests/lds_plan.py and tests/light_plan.py, which take the device's LDS limit.

The case table.  Every frame takes its camera matrix from a 96 x 54 describe() of its scene and is rendered at the extreme size: the
picture is stretched, not cropped, so a frame 70001 rows high has sky at the top, spheres in the middle and ground at the bottom
(test_plan_frame_extremes.py asserts it: at least 5 % of the pixels differ from the sky-only frame and at least 5 % are sky; a frame ONE
row high is the row at the camera's horizon and has no sky, so only the first half is asked of it).  The builds are
tests/partition_cases.py's, with one more.  A frame's reference is its build's — oracle.render, box_reference, light_reference,
direct_reference — computed once per process and shared.

What the references cost, measured on eight CPU threads (seconds): the
scalar-register and resident frames at 64 samples 0.2 - 0.3 at 3 x 70001, 1.0 at 1 x 131070 and 65537 x 3, 0.7 at 70001 x 1, 2.5 at
262145 x 1; 1 x 65537 at 256 samples 0.3; the hierarchy 2.2 at 3 x 70001 and 5.5 at 70001 x 1; the 1500-sphere field at 2 samples 0.4
and 1.0; the preview 0.01.  The box tree took 3.6 and 9.0 at 64 samples: it is rendered at 32.  The whole table: 40 s.  The restatements of
the post-process calls at 32768 x 3 and 3 x 32768, the largest of their frames: the composed guide 0.8, the filter 0.15 (three iteration
counts together), two reprojection steps with their guides and means 1.9, both upsampling factors 0.35, the three tone curves 0.01."""
import functools
import shutil
import subprocess
import tempfile

import rt_amd
from oracle import binding as oracle
from rt_amd import capi
from tests import lds_plan, light_plan
from tests import partition_cases as pc
from tests.conftest import ROOT

CSRC = ROOT / "rt_amd" / "csrc"
NATIVE = ROOT / "tests" / "native"
# name -> (sources next to tests/native/<name>.cpp, extra compiler flags): as the tests that own them build them
DUMPERS = {
    "launch_plan_dump": (["launch_plan.cpp"], []),
    "box_plan_dump": (["launch_plan.cpp", "frame_setup.cpp"], ["-ffp-contract=off"]),
    "light_plan_dump": (["launch_plan.cpp", "frame_setup.cpp", "lights.cpp"], ["-ffp-contract=off"]),
    "direct_plan_dump": (["launch_plan.cpp", "frame_setup.cpp", "lights.cpp"], ["-ffp-contract=off"]),
    "sky_band_dump": (["sky_band.cpp", "frame_setup.cpp"], ["-ffp-contract=off"]),
}


def have_compiler():
    return shutil.which("g++") is not None


@functools.lru_cache(maxsize=None)
def executable(name):
    sources, extra = DUMPERS[name]
    exe = tempfile.mkdtemp(prefix=name + "_") + "/" + name
    built = subprocess.run(["g++", "-std=c++17", "-O2", *extra, "-Wall", "-Wextra", "-Werror", str(NATIVE / (name + ".cpp")), *(str(CSRC / s) for s in sources), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def run(name, requests):
    """One output line per request (launch_plan_dump: under its header line)."""
    out = subprocess.run([executable(name)], input="".join(" ".join(str(v) for v in r) + "\n" for r in requests), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines()


def table_rows(requests):
    """launch_plan_dump: (n_spheres n_planes planes_tame width local_rows samples_per_pixel camera flags host_frame fast) -> one dict per request"""
    requests = list(requests)
    lines = run("launch_plan_dump", requests)
    names = [n for n in lines[0][2:].split() if n != "|"]
    rows = [dict(zip(names, (int(v) for v in line.split() if v != "|"))) for line in lines[1:]]
    assert len(rows) == len(requests) and all(len(r) == len(names) for r in rows)
    return rows


def named_rows(name, requests):
    """box_plan_dump, light_plan_dump, direct_plan_dump: one dict of the plan's fields per request, or the refusal's line as a string"""
    requests = list(requests)
    lines = run(name, requests)
    assert len(lines) == len(requests)
    return [line if line.startswith("refused ") else {k: int(v) for k, v in (f.split("=") for f in line.split())} for line in lines]


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
SEED = pc.SEED
CAMERA_SIZE = (96, 54)  # every frame's camera matrix is its scene's at this size
TALL, WIDE = (3, 70001), (70001, 1)  # one row past the last whole tile at 70000 rows; a ragged last workgroup of four tiles side by side
SM = capi.RT_HIP_FLAG_SM_MATERIALS

# the builds of tests/partition_cases.py and one it has no use for: the scalar-register kernel under the sm table
EXTRA_BUILDS = [
    pc.Build("small_sm", "scalar-register", pc.named("dielectric"), SM, "oracle", (64,), (None, None, 0)),
]
BUILDS = {**pc.BY_NAME, **{build.name: build for build in EXTRA_BUILDS}}

# (build, samples): the families of the one-shot frames, each rendered at TALL and WIDE into a page-locked host frame and into HBM
FAMILIES = [
    ("small_auto", 64), ("small_half", 64), ("small_sm", 64),
    ("resident_pinhole", 64), ("resident_general", 64),
    ("tiled", 2), ("streamed", 2),
    ("bvh_mg", 64),
    ("boxes_resident", 64), ("boxes_tree", 32),  # (the tree's reference at 64 samples: 9 s at 70001 x 1)
    ("lights_resident", 64), ("direct_resident", 64),
]  # fmt: skip
# (build, samples, size): the shapes of the scalar-register kernel beyond the two above
SHAPES = [
    ("small_auto", 64, (1, 65537)), ("small_auto", 64, (1, 131070)),  # the rows whose one-row tiles were out of range
    ("small_auto", 20, TALL),  # a ragged last chunk; half chunks
    ("small_auto", 256, (1, 65537)),  # four-pixel tiles
    ("small_auto", 16, WIDE), ("small_auto", 16, (65537, 3)), ("small_auto", 16, (262145, 1)), ("small_auto", 64, (65537, 3)), ("small_auto", 64, (262145, 1)),
    ("small_auto", 64, (7, 9)),  # smaller than one tile in both directions
]  # fmt: skip
ONE_SHOT = [(name, spp, size) for name, spp in FAMILIES for size in (TALL, WIDE)] + SHAPES

# What plan_launch gives every frame of the table: (kernel, tile width, tile height) into a page-locked host frame, then into HBM (the
# rolling kernels cut no tiles).  Recorded from the plan; tests/test_plan_frame_extremes.py holds the table to it, the GPU test holds the
# kernel each launch reports to the table.  The host frames of more than 65535 rows are the ones whose one-row tiles (8 x 1, 16 x 1,
# 4 x 1) became two rows high.
S, R, B = "small", "resident", "bvh"
EXPECTED = {
    ("small_auto", 64, TALL): ((S, 4, 2), (S, 4, 2)), ("small_auto", 64, WIDE): ((S, 8, 1), (S, 4, 2)),
    ("small_half", 64, TALL): ((S, 4, 2), (S, 4, 2)), ("small_half", 64, WIDE): ((S, 8, 1), (S, 4, 2)),
    ("small_sm", 64, TALL): ((S, 8, 2), (S, 4, 4)), ("small_sm", 64, WIDE): ((S, 16, 1), (S, 4, 4)),
    ("resident_pinhole", 64, TALL): ((R, 4, 2), (R, 4, 2)), ("resident_pinhole", 64, WIDE): ((R, 8, 1), (R, 4, 2)),
    ("resident_general", 64, TALL): ((R, 4, 2), (R, 4, 2)), ("resident_general", 64, WIDE): ((R, 8, 1), (R, 4, 2)),
    ("tiled", 2, TALL): (("tiled", 0, 0), ("tiled", 0, 0)), ("tiled", 2, WIDE): (("tiled", 0, 0), ("tiled", 0, 0)),
    ("streamed", 2, TALL): (("streamed", 0, 0), ("streamed", 0, 0)), ("streamed", 2, WIDE): (("streamed", 0, 0), ("streamed", 0, 0)),
    ("bvh_mg", 64, TALL): ((B, 4, 2), (B, 4, 2)), ("bvh_mg", 64, WIDE): ((B, 8, 1), (B, 4, 2)),
    ("boxes_resident", 64, TALL): ((R, 8, 2), (R, 4, 4)), ("boxes_resident", 64, WIDE): ((R, 16, 1), (R, 4, 4)),
    ("boxes_tree", 32, TALL): ((B, 16, 2), (B, 8, 4)), ("boxes_tree", 32, WIDE): ((B, 16, 2), (B, 8, 4)),
    ("lights_resident", 64, TALL): ((R, 8, 2), (R, 4, 4)), ("lights_resident", 64, WIDE): ((R, 16, 1), (R, 4, 4)),
    ("direct_resident", 64, TALL): ((R, 8, 2), (R, 4, 4)), ("direct_resident", 64, WIDE): ((R, 16, 1), (R, 4, 4)),
    ("small_auto", 64, (1, 65537)): ((S, 4, 2), (S, 4, 2)), ("small_auto", 64, (1, 131070)): ((S, 4, 2), (S, 4, 2)),
    ("small_auto", 20, TALL): ((S, 8, 2), (S, 4, 4)),
    ("small_auto", 256, (1, 65537)): ((S, 2, 2), (S, 2, 2)),
    ("small_auto", 16, WIDE): ((S, 16, 4), (S, 8, 8)), ("small_auto", 16, (65537, 3)): ((S, 16, 4), (S, 8, 8)), ("small_auto", 16, (262145, 1)): ((S, 16, 4), (S, 8, 8)),
    ("small_auto", 64, (65537, 3)): ((S, 8, 1), (S, 4, 2)), ("small_auto", 64, (262145, 1)): ((S, 8, 1), (S, 4, 2)),
    ("small_auto", 64, (7, 9)): ((S, 8, 1), (S, 4, 2)),
}  # fmt: skip


def case_id(name, spp, size):
    return f"{name}-{spp}spp-{size[0]}x{size[1]}"


@functools.lru_cache(maxsize=None)
def pod_of(name, spp):
    return BUILDS[name].make(spp, *CAMERA_SIZE)


@functools.lru_cache(maxsize=None)
def reference(name, spp, size):
    """(rgba, float mean, stats) of the whole frame from the build's CPU reference: computed once, shared, read-only"""
    build, pod = BUILDS[name], pod_of(name, spp)
    if build.reference == "oracle":
        rgba, rgb, stats = oracle.render(pod, *size, seed=SEED, sm_materials=build.sm, preview=bool(build.flags & pc.PREVIEW))
    elif build.reference == "box":
        rgba, rgb, stats = pc.box_ref.render(pod, *size, seed=SEED, sm_materials=build.sm)
    else:
        rgba, rgb, stats = (pc.direct_ref.render if build.reference == "direct" else pc.light_ref.render)(pod, *size, pc.LIGHT_TABLE, seed=SEED, sm_materials=build.sm)
    rgba.setflags(write=False), rgb.setflags(write=False)
    return rgba, rgb, stats


@functools.lru_cache(maxsize=None)
def sky_only(name, spp, size):
    """the packed frame of the case's camera and samples over an empty scene: what a pixel that sees nothing looks like, jitter for jitter"""
    ivp = pod_of(name, spp).inverse_view_projection[:]
    empty = rt_amd.scene_from_arrays([], [], pc.FIELD_MATERIALS, samples_per_pixel=spp, max_bounces=1, inverse_view_projection=ivp)
    return oracle.render(empty, *size, seed=SEED, want_rgb=False)[0]


@functools.lru_cache(maxsize=None)
def plan(name, spp, size, host, rows=None):
    """plan_launch as the context asks it for the one-shot frame (`rows`: for a share of so many rows), under the MI355X's LDS limit"""
    build, pod = BUILDS[name], pod_of(name, spp)
    rows = size[1] if rows is None else rows
    flags = build.flags & ~pc.DEVICE_BUILD
    camera = pc.camera_of(pod, size)
    if build.table is not None:
        lights, sampled = light_plan.light_counts(pod, pc.LIGHT_TABLE)
        return dict(light_plan.ask((pod.n_spheres, pod.n_planes, size[0], rows, spp, camera, flags, host, lights, sampled, pc.DEVICE_LDS)))
    return lds_plan.plan(pod.n_spheres, pod.n_planes, size[0], rows, spp, n_boxes=pod.n_boxes, camera=camera, flags=flags, host_frame=host, lds_limit=pc.DEVICE_LDS)


def tile_of(p):
    """(kernel name, tile width, tile height); the rolling kernels cut no tiles"""
    kernel = capi.KERNEL_NAMES[p["variant"]]
    return (kernel, 0, 0) if p["big_scene"] else (kernel, 1 << p["tile_w_log2"], 1 << (p["pixels_log2"] - p["tile_w_log2"]))


def band_rows(pod, size):
    """the sky band's rows for a whole one-shot frame of `pod` at `size` (rt_amd/csrc/sky_band.cpp asked on the CPU)"""
    from tests.test_sky_band_rule import request_line

    out = subprocess.run([executable("sky_band_dump")], input=request_line(pod, size) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    (line,) = out.stdout.splitlines()
    return int(dict(field.split("=") for field in line.split()[1:])["rows"])
